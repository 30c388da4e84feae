"""The one-frame FFT body the narrow input formats share (sdrainer_amd/csrc/k_fft_psd.h fft_psd_one_frame, the body of
k_fft_psd_narrow<InSc16 / InIq8, LOGN, false / true>) over the full product of its branches at the smallest shapes:
formats sc16, cs8, cu8; window off and on; every N it is instantiated for; two bands, three frames; no listener, a few
listeners with bins 0 and N - 1 among them (the LDS tap) and, at N = 1024, more than kMaxLdsTap (the tap that re-reads
the stored row); one graph replay per format (the format's trait names the BatchCursor field) - and one more per format
through k_fft_r32 (k_fft_r32.h), which takes its replayed pointer from the same trait.

The library's contract is the expectation: a bank fed the narrow samples gives, bit for bit, what a bank fed their
float32 values through the float32 call gives - every psd and spectrum row, every listener's tapped value (the traced
value is a function of it alone), frame record and delivery.  The samples are uniform over the format's whole range.

The same pair of banks serves two more kernel templates: phase A of the two-phase FFT (k_fft_2p_a.h k_fft2p_a<LOGN, FMT,
WIN...>) in its narrow instances, and the multi-frame instance of the float32 kernel (k_fft_psd<LOGN, true, WIN...>) against
the one-frame instance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import iq8_tools as t8  # noqa: E402
from parity_tools import capi, environment, planned, random_window, sc16_to_float32  # noqa: E402, F401 (capi, planned: fixtures)

RATE = t8.RATE
BANDS, FRAMES = 2, 3
FORMATS = ["sc16", "cs8", "cu8"]
SIZES = [512, 1024, 2048, 4096, 8192, 16384]


def samples(fmt, shape, seed):
    """Uniform over every value of the format: int16, int8 or uint8 of the given shape."""
    rng = np.random.default_rng(seed)
    if fmt == "f32":  # (test_multi_frame: both banks take float32)
        return (rng.random(shape, dtype=np.float32) * np.float32(2) - np.float32(1)).astype(np.float32)
    if fmt == "sc16":
        return rng.integers(-32768, 32768, shape, dtype=np.int16)
    x = rng.integers(0, 256, shape, dtype=np.uint8)
    return x.view(np.int8) if fmt == "cs8" else x


def to_f32(fmt, q):
    if fmt == "f32":
        return q
    return sc16_to_float32(q) if fmt == "sc16" else t8.to_f32(q, t8.FORMAT_IDS.index(fmt))


class Pair:
    """Bank a takes the float32 values through the float32 calls, bank b the narrow samples through their format's (fmt
    "f32": the same float32 values).  b_env: switches in the environment while bank b is created, and only then."""

    def __init__(self, capi, n, fmt, window, listeners=8, bands=BANDS, frames=FRAMES, b_env=None):
        self.n, self.fmt, self.bands, self.frames, self.lids = n, fmt, bands, frames, [[] for _ in range(bands)]
        mk = lambda: capi.Bank(RATE[n], n, n_bands=bands, max_batch_frames=frames, max_listeners=listeners, trace=True)
        self.a = mk()
        with environment(**(b_env or {})):
            self.b = mk()
        for bk in (self.a, self.b):
            bk.enable_results(True)
            if window:
                bk.set_window(random_window(n, 4000 + n))

    def attach(self, bins):
        for band in range(self.bands):
            for bin_ in bins:
                ia, ib = self.a.attach(band, int(bin_)), self.b.attach(band, int(bin_))
                assert ia == ib >= 0
                self.lids[band].append(ia)

    def device(self, q):
        ta, tb = torch.from_numpy(to_f32(self.fmt, q)).cuda(), torch.from_numpy(np.ascontiguousarray(q)).cuda()
        torch.cuda.synchronize()
        return ta, tb

    def run(self, seed, traced=None, rows=None):
        ta, tb = self.device(samples(self.fmt, (self.bands, self.frames, 2 * self.n), seed))
        self.a.process_device(ta.data_ptr(), self.frames)
        if self.fmt == "f32":
            self.b.process_device(tb.data_ptr(), self.frames)
        elif self.fmt == "sc16":
            self.b.process_device_sc16(tb.data_ptr(), self.frames)
        else:
            self.b.process_device_iq8(tb.data_ptr(), self.frames, t8.FORMAT_IDS.index(self.fmt))
        self.check(traced, rows)

    def check(self, traced=None, rows=None):
        """traced: positions in the attach order whose traces are compared (default: every listener); rows: the frames whose
        psd and spectrum rows are compared (default: every frame)."""
        self.a.sync()
        self.b.sync()
        for band in range(self.bands):
            for f in range(self.frames) if rows is None else rows:
                (sa, pa), (sb, pb) = self.a.read_spectrum(band, f), self.b.read_spectrum(band, f)
                assert pa.tobytes() == pb.tobytes(), f"band {band} frame {f}: psd row differs"
                assert sa.tobytes() == sb.tobytes(), f"band {band} frame {f}: spectrum row differs"
                assert np.all(np.isfinite(pb)) and pb.max() > 0
            assert self.a.read_frame_records(band).tobytes() == self.b.read_frame_records(band).tobytes(), f"band {band}: frame records"
            lids = self.lids[band] if traced is None else [self.lids[band][k] for k in traced]
            for lid in lids:
                va, vb = self.a.read_trace(band, lid), self.b.read_trace(band, lid)
                assert len(va[0]) == self.frames
                for x, y, what in zip(va, vb, ("tapped value", "raw bit", "debounced bit")):
                    assert x.tobytes() == y.tobytes(), f"band {band} listener {lid}: {what} differs"
        assert t8.same_deliveries(self.a, self.b) > 0

    def replay(self, bins, seed):
        """One replay of sdr_graph_batches() captured batches, each with its own input, on both banks."""
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        self.a.set_stream(streams[0].cuda_stream)
        self.b.set_stream(streams[1].cuda_stream)
        self.attach(bins)
        K = self.a.graph_batches
        fmt_id = None if self.fmt == "sc16" else t8.FORMAT_IDS.index(self.fmt)
        self.a.graph_capture(FRAMES)
        if self.fmt == "sc16":
            self.b.graph_capture_sc16(FRAMES)
        else:
            self.b.graph_capture_iq8(FRAMES, fmt_id)
        dev = [self.device(samples(self.fmt, (self.bands, FRAMES, 2 * self.n), seed + k)) for k in range(K)]
        self.a.graph_launch([ta.data_ptr() for ta, _ in dev])
        if self.fmt == "sc16":
            self.b.graph_launch_sc16([tb.data_ptr() for _, tb in dev])
        else:
            self.b.graph_launch_iq8([tb.data_ptr() for _, tb in dev], fmt_id)
        self.check()  # (the read calls see the replay's last batch, the deliveries every batch)
        self.a.graph_release()
        self.b.graph_release()

    def close(self):
        self.a.close()
        self.b.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("window", [False, True], ids=["plain", "win"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_no_listener_then_lds_tap(capi, fmt, window, n):
    """One batch without a listener (no tap), then one with five, bins 0 and N - 1 among them (the tap out of LDS)."""
    p = Pair(capi, n, fmt, window)
    p.run(n + 1)
    p.attach([0, n - 1, n // 2, 37, n - 70])
    p.run(n + 2)
    p.close()


@pytest.mark.parametrize("window", [False, True], ids=["plain", "win"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_drain_tap(capi, fmt, window):
    """N = 1024 with 4100 listeners, more than kMaxLdsTap: the tap re-reads the stored psd row.  Every row, record and
    delivery is compared; the traces of the first listeners (bins 0 and N - 1), of those around slot 4096 and of the last."""
    n, count = 1024, 4100
    p = Pair(capi, n, fmt, window, listeners=count)
    p.attach([0, n - 1] + [(k * 7919) % n for k in range(2, count)])
    p.run(5000, traced=[0, 1, 2, 4094, 4095, 4096, 4097, count - 1])
    p.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_graph_replay(capi, fmt):
    """The narrow format's graph against the float32 graph, N = 2048, one replay of sdr_graph_batches() batches with their own
    inputs: the kernel takes each batch's pointer from the cursor field of its format."""
    n = 2048
    p = Pair(capi, n, fmt, False)
    p.replay([0, n - 1, 300], 6000)
    p.close()


# FftKernel (host/batch_plan.h) of the dense k_fft_r32 instance of each format, by the plan's name for it
R32_IDS = {"f32": ("k_fft_r32", 8), "sc16": ("k_fft_r32_sc16", 9), "cs8": ("k_fft_r32_iq8", 10), "cu8": ("k_fft_r32_iq8", 10)}


@pytest.mark.parametrize("fmt", FORMATS)
def test_graph_replay_r32(capi, planned, fmt):
    """The same through k_fft_r32 (forced with SDR_FFT_R32=1: by itself it starts at 1024 frames): N = 16384, dense, one
    band, two listeners, three frames per batch, one replay.  Both graphs run the k_fft_r32 instance of their format, and
    the narrow one takes each batch's pointer from the cursor field its trait names.  (Hopped banks refuse graph capture:
    the strided instances have no cursor path.)"""
    n = 16384
    with environment(SDR_FFT_R32=1):
        for f in ("f32", fmt):
            assert planned(n, FRAMES, 2, False, f, 0) == R32_IDS[f] + (0,)
        p = Pair(capi, n, fmt, False, bands=1)
        p.replay([0, n - 1], 6100)
        p.close()


# FftKernel (host/batch_plan.h): the first id of each family; the two-phase ids add the format's number
PSD, PSD_MULTI, PSD_WIN, PSD_WIN_MULTI, A2P, A2P_WIN = 0, 1, 4, 5, 14, 18
FORMAT_NUMBER = {"f32": 0, "sc16": 1, "cs8": 2, "cu8": 3}


@pytest.mark.parametrize("n", [32768, 65536])
@pytest.mark.parametrize("window", [False, True], ids=["plain", "win"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_two_phase(capi, planned, fmt, window, n):
    """Phase A's narrow instances, k_fft2p_a<LOGN, SC16 / CS8 / CU8> plain and windowed, against its float32 instance: two
    bands, three frames (one frame group), a batch without a listener, then one with five, bins 0 and N - 1 among them."""
    name, first = ("k_fft2p_win_a", A2P_WIN) if window else ("k_fft2p_a", A2P)
    for slots in (0, 5):
        for f in ("f32", fmt):
            assert planned(n, FRAMES, slots, window, f, 0) == (name, first + FORMAT_NUMBER[f], 0)
    p = Pair(capi, n, fmt, window)
    p.run(n + 3)
    p.attach([0, n - 1, n // 2, 37, n - 70])
    p.run(n + 4)
    p.close()


@pytest.mark.parametrize("window", [False, True], ids=["plain", "win"])
def test_multi_frame(capi, planned, window):
    """The float32 kernel's multi-frame instance against its one-frame instance on the same input: N = 512, one band, 515
    frames, five listeners.  Bank a is created with the environment as it is and runs one frame per workgroup; bank b is
    created under SDR_FFT_FPW=2 and runs 258 workgroups of two frames, the last with a single frame.  Frame records, traces
    and deliveries are compared in full, the psd rows at both ends of the batch."""
    n, frames, bins = 512, 515, [0, 511, 256, 37, 442]
    name = "k_fft_psd_win" if window else "k_fft_psd"
    assert planned(n, frames, len(bins), window, "f32", 0) == (name, PSD_WIN if window else PSD, 1)
    with environment(SDR_FFT_FPW=2):
        assert planned(n, frames, len(bins), window, "f32", 0) == (name, PSD_WIN_MULTI if window else PSD_MULTI, 2)
    p = Pair(capi, n, "f32", window, bands=1, frames=frames, b_env={"SDR_FFT_FPW": 2})
    p.attach(bins)
    p.run(7000, rows=[0, 1, 2, 513, 514])
    p.close()
