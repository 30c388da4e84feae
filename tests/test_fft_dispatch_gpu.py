"""The one FFT dispatch (sdrainer_amd/csrc/fft_launch.hip launch_fft over host/batch_plan.h fft_kernel): one case per
kernel id, each asserted by name through the host helper (tests/host/iq8_plan.cpp) and then run through the parity driver
on a bank with trace - psd and spectrum rows, tap values, raw and debounced bits, frame records, edges and runes bit for bit
against the CPU oracle.  A mis-wired arm shows as wrong bits: another format or a missing window changes every psd value,
another frame stride every frame after the first.

The shapes are the smallest at which an arm can go wrong: three frames and two listeners for the one-frame kernels and for
k_fft_r32 (forced with SDR_FFT_R32=1: by itself it starts at 1024 frames), two frames of 32768 points for the two phases,
and 515 frames of 512 points at SDR_FFT_FPW=2 for the multi-frame workgroup - 258 workgroups, so the halving rule keeps 2,
and the odd count leaves the last workgroup one frame."""
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import iq8_tools as t8  # noqa: E402
from parity_case import Case  # noqa: E402
from parity_tools import RATES, capi, environment, listener_bins, make_stream, planned, random_window  # noqa: E402, F401 (capi, planned: fixtures)

FORMATS = ("f32", "sc16", "cs8", "cu8")
PATH = {"f32": "device", "sc16": "device_sc16", "cs8": "device_cs8", "cu8": "device_cu8"}
IQ8 = {"cs8": t8.CS8, "cu8": t8.CU8}


def run_case(capi, n, frames, listeners, fmt, hop, windowed, seed):
    """One band, one batch: `frames` frames of format fmt at hop `hop` (0: dense), with a random window or without."""
    if fmt in IQ8:
        q, bins = t8.stream(n, hop or n, frames, 2, seed, IQ8[fmt])
        band, rate = (t8.to_f32(q, IQ8[fmt]), q, bins), t8.RATE[n]
    else:
        band, rate = make_stream(n, hop or n, frames, RATES[n], 2, seed, fmt == "sc16"), RATES[n]
    window = random_window(n, seed + 1) if windowed else None
    case = Case(n, 1, None, 0, [("batch", frames)], seed, rate=rate, max_listeners=listeners, path=PATH[fmt], bands=[band],
                init_bins=[listener_bins(n, band[2], listeners)], hop=hop, windows=[window], trace=True)
    case.run(capi, activity=False).close()


# FftKernel (host/batch_plan.h), in its order
PSD, PSD_MULTI, PSD_SC16, PSD_IQ8, PSD_WIN, PSD_WIN_MULTI, PSD_SC16_WIN, PSD_IQ8_WIN = range(8)
R32, R32_SC16, R32_IQ8, R32_HOP, R32_HOP_SC16, R32_HOP_IQ8 = range(8, 14)
A2P, A2P_WIN = 14, 18  # + the format's number

PSD_IDS = {("f32", False): ("k_fft_psd", PSD), ("sc16", False): ("k_fft_psd_sc16", PSD_SC16), ("cs8", False): ("k_fft_psd_iq8", PSD_IQ8),
           ("cu8", False): ("k_fft_psd_iq8", PSD_IQ8), ("f32", True): ("k_fft_psd_win", PSD_WIN), ("sc16", True): ("k_fft_psd_sc16_win", PSD_SC16_WIN),
           ("cs8", True): ("k_fft_psd_iq8", PSD_IQ8_WIN), ("cu8", True): ("k_fft_psd_iq8", PSD_IQ8_WIN)}


@pytest.mark.parametrize("windowed", [False, True], ids=["plain", "window"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_psd_family(capi, planned, fmt, windowed):
    name, kid = PSD_IDS[fmt, windowed]
    assert planned(512, 3, 2, windowed, fmt, 0) == (name, kid, 1)
    run_case(capi, 512, 3, 2, fmt, 0, windowed, 11)


@pytest.mark.parametrize("windowed", [False, True], ids=["plain", "window"])
def test_psd_multi_frame(capi, planned, windowed):
    with environment(SDR_FFT_FPW=2):
        assert planned(512, 515, 0, windowed, "f32", 0) == (("k_fft_psd_win", PSD_WIN_MULTI, 2) if windowed else ("k_fft_psd", PSD_MULTI, 2))
        run_case(capi, 512, 515, 0, "f32", 0, windowed, 12)


R32_IDS = {("f32", 0): ("k_fft_r32", R32), ("sc16", 0): ("k_fft_r32_sc16", R32_SC16), ("cs8", 0): ("k_fft_r32_iq8", R32_IQ8),
           ("cu8", 0): ("k_fft_r32_iq8", R32_IQ8), ("f32", 4096): ("k_fft_r32_hop", R32_HOP), ("sc16", 4096): ("k_fft_r32_hop_sc16", R32_HOP_SC16),
           ("cs8", 4096): ("k_fft_r32_hop_iq8", R32_HOP_IQ8), ("cu8", 4096): ("k_fft_r32_hop_iq8", R32_HOP_IQ8)}


@pytest.mark.parametrize("hop", [0, 4096], ids=["dense", "hop4096"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_r32_family(capi, planned, fmt, hop):
    with environment(SDR_FFT_R32=1):
        assert planned(16384, 3, 2, False, fmt, hop) == R32_IDS[fmt, hop] + (0,)
        run_case(capi, 16384, 3, 2, fmt, hop, False, 13)


# (one strided case: the stride is an argument of every phase A alike)
@pytest.mark.parametrize("fmt, windowed, hop", [(f, w, 0) for f in FORMATS for w in (False, True)] + [("cu8", False, 4096)])
def test_two_phase(capi, planned, fmt, windowed, hop):
    want = ("k_fft2p_win_a", A2P_WIN + FORMATS.index(fmt), 0) if windowed else ("k_fft2p_a", A2P + FORMATS.index(fmt), 0)
    assert planned(32768, 2, 2, windowed, fmt, hop) == want
    run_case(capi, 32768, 2, 2, fmt, hop, windowed, 14)
