"""The down-converter's real input formats on the GPU (SDR_DDC_RF32 / _RS16 / _RS8 / _RU8, csrc/k_ddc_real.hip): a real
stream v is the complex stream (v, +0.0f), so the oracle is tests/ddc_ref.py fed ddc_real.as_complex(v), bit for bit
(two NaNs count as equal, as in the fuzz).  Every format over the tile shapes at which the kernel takes another path, cuts
of the stream into calls through both entry points with a retune, the GPU's own float32 complex path fed (v, +0.0f) -
non-finite and signed-zero samples included -, the refusals, and the chain: one real wide stream pushed from host memory
through the DDC into a bank of three bands on the same HIP stream, the third band tuned to the mirror image."""
import ctypes as C

import numpy as np
import pytest

import ddc_real as DR
import ddc_ref as R
from ddc_run import run_gpu
from parity_tools import capi, check_batch_polled, nan_equal_bits, run_oracle  # noqa: F401

pytestmark = pytest.mark.gpu

STEPS = (0, 9000, -32768)
# (D, T, outputs): the smallest geometry; odd D and T; across the 512-output tile; one 64-output chunk plus one
SHAPES = [(1, 1, 5), (3, 7, 23), (8, 64, 513), (256, 4096, 65)]


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


def random_taps(t, seed):
    return np.random.default_rng(seed).uniform(-1, 1, t).astype(np.float32)


def ref_of(raw, fmt):
    """What tests/ddc_ref.py takes for a raw real stream."""
    return DR.as_complex(DR.to_f32_real(raw, fmt))


@pytest.mark.parametrize("fmt", DR.FORMATS, ids=DR.FORMAT_IDS)
@pytest.mark.parametrize("d,t,m", SHAPES)
def test_parity_with_the_reference(capi, table, fmt, d, t, m):
    assert capi.DDC_TILE_OUTPUTS == 512
    taps = random_taps(t, 100 * d + t)
    raw = DR.random_raw_real(d * m, fmt, 7 * d + t + fmt)
    if fmt in (DR.RS8, DR.RU8) and len(raw) >= 256:
        assert len(np.unique(raw)) == 256
    k0 = 12345 * d
    want = R.ddc_ref(ref_of(raw, fmt), d, taps, STEPS, *table, first_sample=k0)
    got = run_gpu(capi, fmt, d, taps, STEPS, [raw], first_sample=k0)
    assert got.shape == (len(STEPS), m, 2)
    assert nan_equal_bits(got, want)
    assert np.count_nonzero(got[1]) >= m  # (the comparison is not one of zeros: band 1 has both parts)


# (D, T, the calls' samples, the call in front of which band 1 is retuned).  D = 3, T = 7: three calls shorter than T - 1,
# two of them consecutive, so a carried sample survives two calls; D = 8, T = 64: the carry is rebuilt from 8 + 56 samples
CUTS = [(3, 7, (3, 9, 3, 3, 21, 30), 4), (8, 64, (8, 56, 8, 4104), 3)]


@pytest.mark.parametrize("fmt", DR.FORMATS, ids=DR.FORMAT_IDS)
@pytest.mark.parametrize("d,t,lens,retune_at", CUTS, ids=["d3t7", "d8t64"])
def test_call_cuts_through_both_entry_points(capi, table, fmt, d, t, lens, retune_at):
    assert sum(n < t - 1 for n in lens) >= 2 and all(n % d == 0 for n in lens)
    taps = random_taps(t, 5)
    raw = DR.random_raw_real(sum(lens), fmt, 900 + fmt)
    cuts = np.cumsum((0,) + tuple(lens))
    pieces = [raw[a:e] for a, e in zip(cuts[:-1], cuts[1:])]
    ref = R.DdcRef(d, taps, list(STEPS), *table)
    want = []
    for i, p in enumerate(pieces):
        if i == retune_at:
            ref.steps[1] = -4001
        want.append(ref.process(ref_of(p, fmt)))
    want = np.concatenate(want, axis=1)
    got = run_gpu(capi, fmt, d, taps, STEPS, pieces, host=[i % 2 == 0 for i in range(len(pieces))],
                  between=lambda ddc, i: i == retune_at and ddc.set_nco_step(1, -4001))
    assert nan_equal_bits(got, want)
    whole_ref = R.ddc_ref(ref_of(raw, fmt), d, taps, STEPS, *table)
    whole = run_gpu(capi, fmt, d, taps, STEPS, [raw])
    assert nan_equal_bits(whole, whole_ref)
    for b in (0, 2):  # the bands that were not retuned: a cut changes no bit
        assert nan_equal_bits(got[b], whole[b])
    assert not nan_equal_bits(got[1], whole[1])  # (the retune did change its band)


def special_f32(n, seed):
    """A float32 stream in [-1, 1) with a run of -0.0, a run of subnormals, and single +-FLT_MAX, +-Inf and NaN samples far
    enough apart that most outputs stay finite."""
    v = DR.random_raw_real(n, DR.RF32, seed)
    fmax = np.finfo(np.float32).max
    v[100:180] = np.float32(-0.0)
    v[300:380] = (np.random.default_rng(seed + 1).uniform(-1, 1, 80) * 1e-39).astype(np.float32)
    for at, x in zip(range(600, n, 350), (fmax, -fmax, np.inf, -np.inf, np.nan, -np.nan, fmax, np.inf)):
        v[at] = np.float32(x)
    assert np.signbit(v[100]) and v[100] == 0 and 0 < np.abs(v[300:380]).max() < np.finfo(np.float32).tiny
    assert np.isnan(v).sum() == 2 and np.isinf(v).sum() == 3
    return v


@pytest.mark.parametrize("fmt", DR.FORMATS, ids=DR.FORMAT_IDS)
def test_real_equals_the_complex_path(capi, fmt):
    """The GPU's real kernel against the GPU's SDR_DDC_F32 kernel fed (value, +0.0f)."""
    d, t, m, steps = 8, 64, 600, (32767, -1)
    taps = random_taps(t, 17)
    raw = special_f32(d * m, 3) if fmt == DR.RF32 else DR.random_raw_real(d * m, fmt, 70 + fmt)
    real = run_gpu(capi, fmt, d, taps, steps, [raw])
    cplx = run_gpu(capi, capi.DDC_F32, d, taps, steps, [ref_of(raw, fmt)])
    assert real.shape == cplx.shape == (2, m, 2)
    assert np.array_equal(np.isnan(real), np.isnan(cplx))
    assert nan_equal_bits(real, cplx)
    if fmt == DR.RF32:
        assert np.isnan(real).any() and np.isfinite(real).sum() > real.size // 2


def test_refusals_change_nothing(capi, table):
    import torch

    L = capi.load()
    vp = C.c_void_p
    d, t, steps = 8, 16, (100, -200)
    taps = random_taps(t, 15)
    tp = taps.ctypes.data_as(C.POINTER(C.c_float))
    st = np.array(steps, np.int32)
    sp = st.ctypes.data_as(C.POINTER(C.c_int32))
    cap = 64 * d
    h = vp()
    for bad in (4, 15, 20, 24, 32, -16):
        cfg = capi.DdcConfig(C.sizeof(capi.DdcConfig), len(steps), d, t, bad, cap, 0, 0)
        h.value = 0xdead
        assert L.sdr_ddc_create(C.byref(cfg), tp, sp, C.byref(h)) == capi.ERR_BAD_ARG, bad
        assert h.value == 0xdead and L.sdr_last_error()

    ddc = capi.Ddc(d, taps, steps, in_format=capi.DDC_RU8, max_in_samples=cap)
    ddc.set_stream(torch.cuda.current_stream().cuda_stream)
    raw_in = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    out = torch.zeros((2, 80, 2), dtype=torch.float32, device="cuda")
    i_ok, o_ok = vp(raw_in.data_ptr()), vp(out.data_ptr())
    assert raw_in.data_ptr() % 16 == 0
    refusals = [
        (capi.ERR_BAD_ARG, L.sdr_ddc_process_device, ddc._h, vp(raw_in.data_ptr() + 8), 8 * d, o_ok, 8),  # 8 bytes off 16
        (capi.ERR_BAD_SIZE, L.sdr_ddc_process_device, ddc._h, i_ok, 12, o_ok, 8),                          # not a multiple of D
        (capi.ERR_BAD_SIZE, L.sdr_ddc_process_device, ddc._h, i_ok, cap + d, o_ok, 80),                    # above the capacity
        (capi.ERR_BAD_SIZE, L.sdr_ddc_process_host, ddc._h, vp(st.ctypes.data), 12, o_ok, 8),
    ]
    piece = 8 * d
    raw = DR.random_raw_real(piece * (len(refusals) + 1), DR.RU8, 16)
    want = R.ddc_ref(ref_of(raw, DR.RU8), d, taps, steps, *table)
    for i in range(len(refusals) + 1):
        if i:
            status, call, *args = refusals[i - 1]
            assert call(*args) == status, (i, L.sdr_last_error())
            assert L.sdr_last_error()
            assert ddc.total_samples == i * piece
        raw_in[:piece] = torch.from_numpy(raw[i * piece:(i + 1) * piece]).cuda()
        ddc.process_device(raw_in.data_ptr(), piece, out.data_ptr(), 80)
        ddc.sync()
        assert ddc.total_samples == (i + 1) * piece
        assert nan_equal_bits(out.cpu().numpy()[:, :8], want[:, 8 * i:8 * i + 8]), f"the good call behind refusal {i}"
    ddc.close()


@pytest.fixture(scope="module")
def e2e_oracle(table):
    """Per quantisation, computed once: the raw stream, the reference's narrow streams and the oracle receivers' outputs."""
    cache = {}

    def get(quantise):
        if quantise not in cache:
            e = DR.E2E_REAL
            raw, narrow = DR.e2e_real_wide(quantise)
            ref = R.ddc_ref(ref_of(raw, DR.QUANTISED[quantise]), e["decimation"], DR.e2e_real_taps(), e["steps"], *table)
            centers = [14_000_000 + int(round(s * e["wide_rate"] / R.L)) for s in e["steps"]]
            _, outs, decs = run_oracle(e["rate"], e["n"], e["edge"], [[b] for b in e["bins"]], list(ref), centers, e["hop"])
            cache[quantise] = (raw, narrow, ref, centers, outs, decs)
        return cache[quantise]
    return get


@pytest.mark.parametrize("quantise", sorted(DR.QUANTISED))
def test_end_to_end_with_a_bank_on_one_stream(capi, e2e_oracle, quantise):
    """real wide stream in host memory -> sdr_ddc_process_host in chunks (D = 8, T = 64) -> a ring in device memory -> bank
    (N = 512, hop 128, sdr_process_device_stream), both on one HIP stream with no host synchronisation between a pair's two
    calls, built like the end-to-end test of tests/test_ddc_gpu.py."""
    import torch

    e = DR.E2E_REAL
    n, hop, rate, d, frames, bands = e["n"], e["hop"], e["rate"], e["decimation"], e["frames"], len(e["steps"])
    raw, narrow, ref, centers, outs, decs = e2e_oracle(quantise)
    taps = DR.e2e_real_taps()
    assert d == 8 and len(taps) == 64 and raw.ndim == 1

    per = 512  # frames' worth of samples per DDC call, at the most
    lens = [min(per * hop, narrow - a) for a in range(0, narrow, per * hop)]
    stride = narrow
    assert stride % 4 == 0
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        out = torch.full((bands, stride, 2), float("nan"), dtype=torch.float32, device="cuda")
    stream.synchronize()
    bank = capi.Bank(rate, n, n_bands=bands, edge_width=e["edge"], max_batch_frames=per, max_listeners=bands, hop=hop)
    ddc = capi.Ddc(d, taps, e["steps"], in_format=DR.QUANTISED[quantise], max_in_samples=per * hop * d)
    bank.set_stream(stream.cuda_stream)
    ddc.set_stream(stream.cuda_stream)
    for b in range(bands):
        bank.set_center_frequency(b, centers[b])
        assert bank.attach(b, e["bins"][b]) == 0
    bank.enable_results(True)
    have = done = 0  # narrow samples produced, frames processed
    batches = []
    for m in lens:
        ddc.process_host(raw[have * d:(have + m) * d], out.data_ptr() + have * 8, stride)
        have += m
        k = (have - n) // hop + 1 - done if have >= n else 0
        assert k > 0
        bank.process_device_stream(out.data_ptr() + done * hop * 8, k, stride)
        batches.append((done, done + k))
        done += k
    ddc.sync()
    bank.sync()
    assert have == narrow and done == frames and len(batches) >= 3 and bank.total_frames == frames
    assert nan_equal_bits(out.cpu().numpy(), ref)
    text = [[""] for _ in range(bands)]
    n_peaks = 0
    for a, z in batches:
        res = bank.poll(wait=True)
        n_peaks += check_batch_polled(res, outs, a, z, 1, text, bands)[1]
    assert bank.poll() is None
    assert n_peaks > 0 and all(len(o["peak_frames"]) >= 3 for o in outs)  # at least three cumulations per band
    for b, call in enumerate(e["calls"]):
        assert text[b][0] == decs[b][0][0] and call in text[b][0], (b, text[b][0])
    ddc.close()
    bank.close()
