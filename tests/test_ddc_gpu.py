"""The down-converter on the GPU (sdr_ddc_*, csrc/k_ddc.hip) against its NumPy restatement tests/ddc_ref.py, bit for bit:
every input format over the decimations and tap counts at which the kernel's tile takes another shape, cuts of the stream
into calls, sample indices across 2^31 and 2^32, a retune between calls, subnormal products, the host entry point, every
refusal, and the chain - one cu8 wide stream through the DDC into a bank on the same HIP stream, cut into whole hops, cut
raggedly, and cut raggedly with a padded band stride - against the oracle receiver fed with the reference's narrow streams.
The seeded fuzz over every tile shape is tests/test_ddc_fuzz_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import ddc_ref as R
from ddc_run import run_gpu
from parity_tools import bits_equal, capi, check_batch_polled, run_oracle  # noqa: F401

pytestmark = pytest.mark.gpu

STEPS = (0, 9000, -32768)
GEOMETRY = [(1, 1), (1, 5), (2, 3), (3, 7), (5, 4), (8, 64), (64, 1024), (256, 4096)]


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


def random_taps(t, seed):
    return np.random.default_rng(seed).uniform(-1, 1, t).astype(np.float32)


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


def ragged_lengths(narrow, hop):
    """DDC call lengths in outputs, drawn with a fixed seed, as a receiver's are: each even (the next call's output pointer
    stays 16-byte aligned), none a multiple of the hop, a third of them shorter than a hop - after which the bank often has
    no whole new frame."""
    rng = np.random.default_rng(20_241)
    lens, left = [], narrow
    while left > 0:
        m = 2 * int(rng.integers(1, hop // 2) if rng.random() < 0.35 else rng.integers(hop, 100 * hop))
        m += 2 * (m % hop == 0)
        lens.append(min(m, left))
        left -= lens[-1]
    assert all(m % 2 == 0 for m in lens) and all(m % hop for m in lens[:-1]) and sum(lens) == narrow
    return lens


def chain(capi, table, lens=None, gap=0):
    """cu8 wide stream -> DDC (D = 8, T = 64) -> bank (N = 512, hop 128, sdr_process_device_stream), both on one HIP stream,
    call pairs back to back with no host synchronisation between a pair's two calls and one at the end.  lens: the DDC
    calls' outputs (by default 512 frames' worth each); the bank takes whatever whole frames exist behind each and is
    skipped where there is none.  gap: words between one band's narrow stream and the next, which stay as they were."""
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

    per = 512  # frames' worth of samples per DDC call, at the most
    if lens is None:
        lens = [min(per * hop, narrow - a) for a in range(0, narrow, per * hop)]
    assert sum(lens) == narrow and max(lens) <= per * hop
    stride = narrow + gap
    assert stride % 4 == 0
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        wide = torch.from_numpy(raw).cuda()
        out = torch.full((2, stride, 2), float("nan"), dtype=torch.float32, device="cuda")
    stream.synchronize()
    bank = capi.Bank(rate, n, n_bands=2, edge_width=e["edge"], max_batch_frames=per, max_listeners=2, hop=hop)
    ddc = capi.Ddc(d, taps, e["steps"], in_format=capi.DDC_CU8, max_in_samples=per * hop * d)
    bank.set_stream(stream.cuda_stream)
    ddc.set_stream(stream.cuda_stream)
    for b in range(2):
        bank.set_center_frequency(b, centers[b])
        assert bank.attach(b, e["bins"][b]) == 0
    bank.enable_results(True)
    have = done = skipped = 0  # narrow samples produced, frames processed, DDC calls behind which the bank had no new frame
    batches = []
    for m in lens:
        ddc.process_device(wide.data_ptr() + have * d * 2, m * d, out.data_ptr() + have * 8, stride)
        have += m
        k = (have - n) // hop + 1 - done if have >= n else 0
        if k == 0:
            skipped += 1
            continue
        bank.process_device_stream(out.data_ptr() + done * hop * 8, k, stride)
        batches.append((done, done + k))
        done += k
    ddc.sync()
    bank.sync()
    assert have == narrow and done == frames and len(batches) >= 3 and bank.total_frames == frames
    got = out.cpu().numpy()
    assert bits_equal(got[:, :narrow], ref)
    assert np.isnan(got[:, narrow:]).all(), "the words between the bands were written"
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
    return skipped


def test_end_to_end_with_a_bank_on_one_stream(capi, table):
    """Every DDC call makes a whole number of hops."""
    assert chain(capi, table) == 0


def test_end_to_end_with_ragged_calls(capi, table):
    """The same stream cut as a receiver cuts it (ragged_lengths): the same samples, peaks, edges and text."""
    lens = ragged_lengths(R.e2e_wide()[1], R.E2E["hop"])
    assert len(lens) >= 8
    assert chain(capi, table, lens) >= 2  # (calls behind which the bank was skipped)


def test_end_to_end_with_ragged_calls_and_a_band_stride(capi, table):
    """And with the band stride larger than the narrow length: the words between the bands stay untouched."""
    assert chain(capi, table, ragged_lengths(R.e2e_wide()[1], R.E2E["hop"]), gap=64) >= 2
