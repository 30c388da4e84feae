"""The down-converter on the GPU (sdr_ddc_*, csrc/k_ddc.hip) against its NumPy restatement tests/ddc_ref.py, bit for bit:
every input format over the decimations and tap counts at which the kernel's tile takes another shape, cuts of the stream
into calls, sample indices across 2^31 and 2^32, a retune between calls, subnormal products, the host entry point, every
refusal, and the chain - one cu8 wide stream through the DDC into a bank on the same HIP stream - against the oracle
receiver fed with the reference's narrow streams."""
import ctypes as C

import numpy as np
import pytest

import ddc_ref as R
from parity_tools import bits_equal, capi, check_batch_polled, run_oracle  # noqa: F401

pytestmark = pytest.mark.gpu

STEPS = (0, 9000, -32768)
GEOMETRY = [(1, 1), (1, 5), (2, 3), (3, 7), (5, 4), (8, 64), (64, 1024), (256, 4096)]


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


def random_taps(t, seed):
    return np.random.default_rng(seed).uniform(-1, 1, t).astype(np.float32)


def run_gpu(capi, fmt, d, taps, steps, pieces, first_sample=None, between=None, host=False):
    """One DDC over the raw pieces, one call each, every call with device tensors of its own (a call's pointers are 16-byte
    aligned whatever the pieces' lengths); between(ddc, i) runs in front of call i.  Returns float32 [bands, outputs, 2].
    The words behind a band's outputs, up to the band stride, must be left alone."""
    import torch

    ddc = capi.Ddc(d, taps, steps, in_format=fmt, max_in_samples=max(len(p) for p in pieces))
    ddc.set_stream(torch.cuda.current_stream().cuda_stream)
    if first_sample is not None:
        ddc.set_first_sample(first_sample)
    start = ddc.total_samples
    outs = []
    for i, raw in enumerate(pieces):
        if between:
            between(ddc, i)
        m = len(raw) // d
        stride = (m + 3) // 4 * 4 + 4
        out = torch.full((len(steps), stride, 2), float("nan"), dtype=torch.float32, device="cuda")
        if host:
            ddc.process_host(raw, out.data_ptr(), stride)
        else:
            dev = torch.from_numpy(np.ascontiguousarray(raw)).cuda()
            ddc.process_device(dev.data_ptr(), len(raw), out.data_ptr(), stride)
        outs.append((out, m))
    ddc.sync()
    assert ddc.total_samples == start + sum(len(p) for p in pieces)
    ddc.close()
    got = [o.cpu().numpy() for o, _ in outs]
    for g, (_, m) in zip(got, outs):
        assert np.isnan(g[:, m:]).all(), "the kernel wrote behind a band's outputs"
    return np.concatenate([g[:, :m] for g, (_, m) in zip(got, outs)], axis=1)


@pytest.mark.parametrize("fmt", R.FORMATS, ids=R.FORMAT_IDS)
@pytest.mark.parametrize("d,t", GEOMETRY)
def test_parity_with_the_reference(capi, table, fmt, d, t):
    tile = capi.DDC_TILE_OUTPUTS
    counts = (tile - 1, tile, tile + 1, 2 * tile + 37)  # one below, at and one above a tile; three tiles
    taps = random_taps(t, 100 * d + t)
    raw = R.random_raw(d * max(counts), fmt, 7 * d + t + fmt)
    want = R.ddc_ref(R.to_f32(raw, fmt), d, taps, STEPS, *table)
    for m in counts:
        got = run_gpu(capi, fmt, d, taps, STEPS, [raw[:m * d]])
        assert got.shape == (len(STEPS), m, 2)
        assert bits_equal(got, want[:, :m]), f"{m} outputs"


@pytest.mark.parametrize("fmt", R.FORMATS, ids=R.FORMAT_IDS)
@pytest.mark.parametrize("d,t", [(6, 48), (8, 64), (64, 1024)])
def test_call_cuts(capi, table, fmt, d, t):
    """Calls of D and 5 D samples, two consecutive calls shorter than T - 1 (part of the carry survives each), the rest."""
    taps = random_taps(t, 5)
    short = (t - 1) // d // 2 * d
    assert 0 < short < t - 1
    lens = [d, 5 * d, short, short, 700 * d]
    raw = R.random_raw(sum(lens), fmt, 900 + fmt)
    cuts = np.cumsum([0] + lens)
    want = R.ddc_ref(R.to_f32(raw, fmt), d, taps, STEPS, *table)
    whole = run_gpu(capi, fmt, d, taps, STEPS, [raw])
    cut = run_gpu(capi, fmt, d, taps, STEPS, [raw[a:e] for a, e in zip(cuts[:-1], cuts[1:])])
    assert bits_equal(whole, want) and bits_equal(cut, want)


@pytest.mark.parametrize("edge", [2 ** 31, 2 ** 32], ids=["2^31", "2^32"])
def test_large_sample_index(capi, table, edge):
    """The calls cross k = edge; one band has an odd step and one step -1: the phase comes from the full 64-bit index."""
    d, t, steps = 8, 24, (12345, -1, 9000)
    taps = random_taps(t, 11)
    k0 = edge - 50 * d
    lens = [40 * d, 40 * d, 30 * d]  # the second call crosses the edge
    raw = R.random_raw(sum(lens), R.SC16, 31)
    cuts = np.cumsum([0] + lens)
    want = R.ddc_ref(R.to_f32(raw, R.SC16), d, taps, steps, *table, first_sample=k0)
    got = run_gpu(capi, R.SC16, d, taps, steps, [raw[a:e] for a, e in zip(cuts[:-1], cuts[1:])], first_sample=k0)
    assert bits_equal(got, want)
    # (samples below k0 are zero: the first outputs see fewer than T samples, as at index 0)
    assert bits_equal(got[2][0], (taps[0] * R.mix(R.to_f32(raw[:1], R.SC16), np.array([k0]), 9000, *table))[0])


def test_retune_between_calls(capi, table):
    d, t = 8, 64
    taps = random_taps(t, 12)
    lens = [64 * d, 3 * d, 200 * d]
    raw = R.random_raw(sum(lens), R.CS8, 32)
    cuts = np.cumsum([0] + lens)
    pieces = [raw[a:e] for a, e in zip(cuts[:-1], cuts[1:])]
    retune = {1: (0, -4000), 2: (2, 77)}  # in front of call i: (band, step)
    ref = R.DdcRef(d, taps, list(STEPS), *table)
    want = []
    for i, p in enumerate(pieces):
        if i in retune:
            ref.steps[retune[i][0]] = retune[i][1]
        want.append(ref.process(R.to_f32(p, R.CS8)))
    got = run_gpu(capi, R.CS8, d, taps, STEPS, pieces, between=lambda ddc, i: i in retune and ddc.set_nco_step(*retune[i]))
    assert bits_equal(got, np.concatenate(want, axis=1))
    assert not bits_equal(got, R.ddc_ref(R.to_f32(raw, R.CS8), d, taps, STEPS, *table))  # (the retunes did change the bands)


def test_subnormal_products_are_kept(capi, table):
    d, t = 4, 32
    rng = np.random.default_rng(13)
    taps = (rng.uniform(-1, 1, t) * 1e-10).astype(np.float32)
    raw = (rng.uniform(-1, 1, (d * 600, 2)) * 1e-30).astype(np.float32)
    want = R.ddc_ref(raw, d, taps, STEPS, *table)
    tiny = np.finfo(np.float32).tiny
    assert np.all(np.abs(want) < tiny) and np.count_nonzero(want) > want.size * 0.9  # every output is subnormal, few are zero
    assert bits_equal(run_gpu(capi, R.F32, d, taps, STEPS, [raw]), want)


@pytest.mark.parametrize("fmt", R.FORMATS, ids=R.FORMAT_IDS)
def test_host_entry_point_equals_device(capi, table, fmt):
    d, t = 5, 40
    taps = random_taps(t, 14)
    raw = R.random_raw(d * 900, fmt, 50 + fmt)
    pieces = [raw[:d * 300], raw[d * 300:d * 303], raw[d * 303:]]
    dev = run_gpu(capi, fmt, d, taps, STEPS, pieces)
    host = run_gpu(capi, fmt, d, taps, STEPS, pieces, host=True)
    assert bits_equal(host, dev) and bits_equal(dev, R.ddc_ref(R.to_f32(raw, fmt), d, taps, STEPS, *table))


def test_refusals_change_nothing(capi, table):
    import torch

    L = capi.load()
    vp = C.c_void_p
    d, t, steps = 4, 16, (100, -200)
    taps = random_taps(t, 15)
    tp = taps.ctypes.data_as(C.POINTER(C.c_float))
    st = np.array(steps, np.int32)
    sp = st.ctypes.data_as(C.POINTER(C.c_int32))
    cap = 64 * d

    def config(**kw):
        c = capi.DdcConfig(C.sizeof(capi.DdcConfig), len(steps), d, t, capi.DDC_CU8, cap, 0, 0)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    h = vp()
    ddc = capi.Ddc(d, taps, steps, in_format=capi.DDC_CU8, max_in_samples=cap)
    ddc.set_stream(torch.cuda.current_stream().cuda_stream)
    ddc.set_first_sample(8 * d)
    raw_in = torch.zeros((cap + 8, 2), dtype=torch.uint8, device="cuda")
    out = torch.zeros((2, 80, 2), dtype=torch.float32, device="cuda")
    i_ok, o_ok = vp(raw_in.data_ptr()), vp(out.data_ptr())
    big = st.copy()
    big[1] = 32768
    refusals = [
        (capi.ERR_BAD_ARG, L.sdr_ddc_create, C.byref(config(struct_size=28)), tp, sp, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_ddc_create, C.byref(config(decimation=0)), tp, sp, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_ddc_create, C.byref(config(decimation=257, max_in_samples=257)), tp, sp, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_ddc_create, C.byref(config(n_taps=0)), tp, sp, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_ddc_create, C.byref(config(n_taps=4097)), tp, sp, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_ddc_create, C.byref(config(n_bands=0)), tp, sp, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_ddc_create, C.byref(config(n_bands=65)), tp, sp, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_ddc_create, C.byref(config(in_format=4)), tp, sp, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_ddc_create, C.byref(config(in_format=-1)), tp, sp, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_ddc_create, C.byref(config(max_in_samples=cap + 1)), tp, sp, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_ddc_create, C.byref(config(reserved=1)), tp, sp, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_ddc_create, C.byref(config()), None, sp, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_ddc_create, C.byref(config()), tp, None, C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_ddc_create, C.byref(config()), tp, big.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_ddc_process_device, ddc._h, vp(raw_in.data_ptr() + 2), 8 * d, o_ok, 8),   # misaligned input
        (capi.ERR_BAD_ARG, L.sdr_ddc_process_device, ddc._h, i_ok, 8 * d, vp(out.data_ptr() + 8), 8),      # misaligned output
        (capi.ERR_BAD_ARG, L.sdr_ddc_process_device, ddc._h, None, 8 * d, o_ok, 8),
        (capi.ERR_BAD_ARG, L.sdr_ddc_process_device, ddc._h, i_ok, 8 * d, None, 8),
        (capi.ERR_BAD_SIZE, L.sdr_ddc_process_device, ddc._h, i_ok, 8 * d + 1, o_ok, 12),  # not a multiple of D
        (capi.ERR_BAD_SIZE, L.sdr_ddc_process_device, ddc._h, i_ok, 0, o_ok, 8),
        (capi.ERR_BAD_SIZE, L.sdr_ddc_process_device, ddc._h, i_ok, cap + d, o_ok, 80),    # above the capacity
        (capi.ERR_BAD_ARG, L.sdr_ddc_process_device, ddc._h, i_ok, 8 * d, o_ok, 4),        # a stride below the outputs
        (capi.ERR_BAD_ARG, L.sdr_ddc_process_device, ddc._h, i_ok, 8 * d, o_ok, 10),       # not a multiple of 4
        (capi.ERR_BAD_SIZE, L.sdr_ddc_process_host, ddc._h, vp(st.ctypes.data), d + 1, o_ok, 8),
        (capi.ERR_BAD_ARG, L.sdr_ddc_set_nco_step, ddc._h, 2, 5),
        (capi.ERR_BAD_ARG, L.sdr_ddc_set_nco_step, ddc._h, -1, 5),
        (capi.ERR_BAD_ARG, L.sdr_ddc_set_nco_step, ddc._h, 0, 32768),
        (capi.ERR_BAD_ARG, L.sdr_ddc_set_nco_step, ddc._h, 0, -32769),
        (capi.ERR_STATE, L.sdr_ddc_set_first_sample, ddc._h, 16 * d),  # (after the first good call, below)
    ]
    assert L.sdr_ddc_set_first_sample(ddc._h, -d) == capi.ERR_BAD_ARG and L.sdr_ddc_set_first_sample(ddc._h, 8 * d + 1) == capi.ERR_BAD_ARG
    assert ddc.total_samples == 8 * d
    # a good call of 8 outputs in front of the first refusal and behind every one: the stream goes on as if nothing was tried
    piece = 8 * d
    raw = R.random_raw(piece * (len(refusals) + 1), R.CU8, 16)
    want = R.ddc_ref(R.to_f32(raw, R.CU8), d, taps, steps, *table, first_sample=8 * d)
    for i in range(len(refusals) + 1):
        if i:
            status, call, *args = refusals[-i]
            h.value = 0xdead
            assert call(*args) == status, (i, L.sdr_last_error())
            assert h.value == 0xdead and L.sdr_last_error()
            assert ddc.total_samples == 8 * d + i * piece
        raw_in[:piece] = torch.from_numpy(raw[i * piece:(i + 1) * piece]).cuda()
        ddc.process_device(raw_in.data_ptr(), piece, out.data_ptr(), 80)
        ddc.sync()
        assert bits_equal(out.cpu().numpy()[:, :8], want[:, 8 * i:8 * i + 8]), f"the good call behind refusal {i}"
    ddc.close()


def test_end_to_end_with_a_bank_on_one_stream(capi, table):
    """cu8 wide stream -> DDC (D = 8, T = 64) -> bank (N = 512, hop 128, sdr_process_device_stream), both on one HIP stream,
    call pairs back to back with no host synchronisation between a pair's two calls and one at the end."""
    import torch

    e = R.E2E
    n, hop, rate, d, frames = e["n"], e["hop"], e["rate"], e["decimation"], e["frames"]
    raw, narrow = R.e2e_wide()
    taps = R.e2e_taps()
    assert d == 8 and len(taps) == 64
    ref = R.ddc_ref(R.to_f32(raw, R.CU8), d, taps, e["steps"], *table)
    centers = [14_000_000 + int(round(s * e["wide_rate"] / R.L)) for s in e["steps"]]
    bins = [[b] for b in e["bins"]]
    _, outs, decs = run_oracle(rate, n, e["edge"], bins, list(ref), centers, hop)

    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        wide = torch.from_numpy(raw).cuda()
        out = torch.zeros((2, narrow, 2), dtype=torch.float32, device="cuda")
    stream.synchronize()
    per = 512  # frames' worth of samples per DDC call
    bank = capi.Bank(rate, n, n_bands=2, edge_width=e["edge"], max_batch_frames=per, max_listeners=2, hop=hop)
    ddc = capi.Ddc(d, taps, e["steps"], in_format=capi.DDC_CU8, max_in_samples=per * hop * d)
    bank.set_stream(stream.cuda_stream)
    ddc.set_stream(stream.cuda_stream)
    for b in range(2):
        bank.set_center_frequency(b, centers[b])
        assert bank.attach(b, e["bins"][b]) == 0
    bank.enable_results(True)
    have = done = 0  # narrow samples produced, frames processed
    batches = []
    while have < narrow:
        m = min(per * hop, narrow - have)
        ddc.process_device(wide.data_ptr() + have * d * 2, m * d, out.data_ptr() + have * 8, narrow)
        have += m
        k = (have - n) // hop + 1 - done
        bank.process_device_stream(out.data_ptr() + done * hop * 8, k, narrow)
        batches.append((done, done + k))
        done += k
    ddc.sync()
    bank.sync()
    assert done == frames and len(batches) >= 3 and bank.total_frames == frames
    assert bits_equal(out.cpu().numpy(), ref)
    text = [[""], [""]]
    n_peaks = 0
    for a, z in batches:
        res = bank.poll(wait=True)
        n_peaks += check_batch_polled(res, outs, a, z, 1, text, 2)[1]
    assert bank.poll() is None
    assert n_peaks > 0 and sum(len(o["peak_frames"]) for o in outs) >= 6  # at least three cumulations per band
    for b, call in enumerate(e["calls"]):
        assert text[b][0] == decs[b][0][0] and call in text[b][0], text[b][0]
    ddc.close()
    bank.close()
