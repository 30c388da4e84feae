"""The polyphase channelizer on the GPU (sdr_chan_*, csrc/k_chan.hip) against its NumPy restatement tests/chan_ref.py, bit for
bit: output counts around a tile for every geometry class and every input format, channel selection with a padded band
stride, cuts of the stream into calls, sample indices across 2^31 and 2^32, subnormal products and non-finite values in
every branch, the host entry point, every refusal, and the chain - one cu8 wide stream through the channelizer into a bank
on the same HIP stream, cut into whole hops and cut raggedly - against the oracle receiver fed with the reference's narrow
streams."""
import ctypes as C

import numpy as np
import pytest

import chan_ref as CR
import ddc_ref as R
from chan_run import run_gpu
from parity_tools import bits_equal, capi, check_batch_polled, nan_equal_bits, run_oracle  # noqa: F401

pytestmark = pytest.mark.gpu

GEOMETRY = [(2, 2, 1), (2, 1, 3), (4, 1, 5), (8, 8, 8), (8, 4, 4), (16, 4, 3), (32, 8, 2), (64, 64, 1), (64, 32, 8), (128, 32, 4),
            (256, 256, 16), (256, 64, 16)]
ALL_FORMATS_AT = [(8, 4, 4), (64, 32, 8)]
PARITY = [(g, f) for g in GEOMETRY for f in CR.FORMATS if f in (R.F32, R.CU8) or g in ALL_FORMATS_AT]


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


def random_taps(t, seed):
    return np.random.default_rng(seed).uniform(-1, 1, t).astype(np.float32)


def fmt_id(f):
    return CR.FORMAT_IDS[CR.FORMATS.index(f)]


@pytest.mark.parametrize("geometry,fmt", PARITY, ids=["%d-%d-%d-%s" % (*g, fmt_id(f)) for g, f in PARITY])
def test_parity_with_the_reference(capi, table, geometry, fmt):
    m, d, p = geometry
    tile = capi.chan_tile_outputs(m, d, m * p)
    assert tile >= 16
    counts = (1, 2, tile - 1, tile, tile + 1, 2 * tile + 37)
    taps = random_taps(m * p, 100 * m + 10 * d + p)
    raw = CR.random_raw(d * max(counts), fmt, 7 * m + d + fmt)
    want = CR.chan_ref(CR.to_f32(raw, fmt), m, d, taps, *table)  # (a prefix of the stream gives a prefix of the outputs)
    for k in counts:
        got = run_gpu(capi, fmt, m, d, taps, [raw[:k * d]])
        assert got.shape == (m, k, 2)
        assert bits_equal(got, want[:, :k]), f"{k} outputs"


def test_channel_selection_keeps_order_and_leaves_the_gaps(capi, table):
    m, d, p = 16, 4, 3
    channels = (m - 1, 0, 5)
    taps = random_taps(m * p, 21)
    tile = capi.chan_tile_outputs(m, d, m * p)
    raw = CR.random_raw(d * (tile + 21), R.SC16, 22)
    whole = CR.chan_ref(R.to_f32(raw, R.SC16), m, d, taps, *table)
    got = run_gpu(capi, R.SC16, m, d, taps, [raw], channels=channels, gap=40)  # (run_gpu: the gap's words are still NaN)
    assert got.shape == (3, tile + 21, 2) and bits_equal(got, whole[list(channels)])
    assert not bits_equal(got[0], whole[0])


@pytest.mark.parametrize("fmt", [R.F32, R.CU8, CR.RR.RS16], ids=["f32", "cu8", "rs16"])
@pytest.mark.parametrize("m,d,p", [(8, 4, 4), (64, 32, 8), (256, 64, 16)])
def test_call_cuts(capi, table, fmt, m, d, p):
    """Calls of D and 5 D samples, two consecutive calls shorter than T - 1 (part of the carry survives each), the rest."""
    t = m * p
    taps = random_taps(t, 5)
    short = (t - 1) // d // 2 * d
    assert 0 < short < t - 1
    lens = [d, 5 * d, short, short, (capi.chan_tile_outputs(m, d, t) + 200) * d]
    raw = CR.random_raw(sum(lens), fmt, 900 + fmt)
    cuts = np.cumsum([0] + lens)
    want = CR.chan_ref(CR.to_f32(raw, fmt), m, d, taps, *table)
    whole = run_gpu(capi, fmt, m, d, taps, [raw])
    cut = run_gpu(capi, fmt, m, d, taps, [raw[a:e] for a, e in zip(cuts[:-1], cuts[1:])])
    assert bits_equal(whole, want) and bits_equal(cut, want)


@pytest.mark.parametrize("edge", [2 ** 31, 2 ** 32], ids=["2^31", "2^32"])
def test_large_sample_index(capi, table, edge):
    """The calls cross k = edge: the rotation n D mod M and the zeros below the first sample come from the 64-bit index."""
    m, d, p = 16, 4, 3
    taps = random_taps(m * p, 11)
    k0 = edge - 50 * d
    assert k0 % m != 0
    lens = [40 * d, 40 * d, 30 * d]  # the second call crosses the edge
    raw = R.random_raw(sum(lens), R.SC16, 31)
    cuts = np.cumsum([0] + lens)
    want = CR.chan_ref(R.to_f32(raw, R.SC16), m, d, taps, *table, first_sample=k0)
    got = run_gpu(capi, R.SC16, m, d, taps, [raw[a:e] for a, e in zip(cuts[:-1], cuts[1:])], first_sample=k0)
    assert bits_equal(got, want)
    assert not bits_equal(got, CR.chan_ref(R.to_f32(raw, R.SC16), m, d, taps, *table))  # (the rotation did follow k0)


def test_subnormal_products_are_kept(capi, table):
    m, d, p = 8, 4, 4
    rng = np.random.default_rng(13)
    taps = (rng.uniform(-1, 1, m * p) * 1e-10).astype(np.float32)
    raw = (rng.uniform(-1, 1, (d * 600, 2)) * 1e-31).astype(np.float32)
    want = CR.chan_ref(raw, m, d, taps, *table)
    tiny = np.finfo(np.float32).tiny
    assert np.all(np.abs(want) < tiny) and np.count_nonzero(want) > want.size * 0.9  # every output is subnormal, few are zero
    assert bits_equal(run_gpu(capi, R.F32, m, d, taps, [raw]), want)


def test_zeros_infinities_nans_and_extremes_in_every_branch(capi, table):
    """An F32 stream with +-0, +-Inf, NaN, 2^+-100 and subnormals, each at a sample of every residue mod M - so in every
    branch r - over a stretch that crosses a tile edge; some taps are +-0.  Zero signs agree; NaNs are NaNs."""
    m, d, p = 8, 4, 4
    t = m * p
    tile = capi.chan_tile_outputs(m, d, t)
    sub = np.float32(1e-41)
    special = [0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** 100, 2.0 ** -100, -2.0 ** 100, sub, -sub]
    taps = random_taps(t, 17)
    taps[[3, 12]] = 0.0
    taps[[7, 21]] = -0.0
    spacing = 2 * t
    first = 2 * t  # the placements run from here across the tile's edge
    n = first + len(special) * m * spacing + 8 * t
    assert first % m == 0 and n % d == 0
    raw = R.random_raw(n, R.F32, 18)
    raw[n - 6 * t:n - 4 * t] = -0.0  # a stretch of negative zeros, longer than the filter
    raw[n - 3 * t:n - t, 0] = 0.0
    for i in range(len(special) * m):
        k = first + i * spacing + i // len(special)  # residue r = i // len(special) mod M
        assert k % m == i // len(special) and k < n
        raw[k, i % 2] = special[i % len(special)]
        raw[k + t + 5, 1 - i % 2] = special[(i + 3) % len(special)]
    assert first < tile * d < first + len(special) * m * spacing
    with np.errstate(all="ignore"):
        want = CR.chan_ref(raw, m, d, taps, *table)
    assert np.isnan(want).any() and np.isinf(want).any() and np.isfinite(want).mean() > 0.5
    assert (want == 0).any()  # (sums that begin at +0 end at +0 over the zero stretches: a -0 from the GPU would differ)
    assert nan_equal_bits(run_gpu(capi, R.F32, m, d, taps, [raw]), want)


@pytest.mark.parametrize("fmt", CR.FORMATS, ids=CR.FORMAT_IDS)
def test_host_entry_point_equals_device(capi, table, fmt):
    m, d, p = 8, 4, 4
    taps = random_taps(m * p, 14)
    raw = CR.random_raw(d * 900, fmt, 50 + fmt)
    pieces = [raw[:d * 300], raw[d * 300:d * 303], raw[d * 303:]]
    dev = run_gpu(capi, fmt, m, d, taps, pieces)
    host = run_gpu(capi, fmt, m, d, taps, pieces, host=True)
    assert bits_equal(host, dev) and bits_equal(dev, CR.chan_ref(CR.to_f32(raw, fmt), m, d, taps, *table))


def test_refusals_change_nothing(capi, table):
    import torch

    L = capi.load()
    vp = C.c_void_p
    m, d, p, channels = 8, 4, 2, (5, 0)
    t = m * p
    taps = random_taps(t, 15)
    tp = taps.ctypes.data_as(C.POINTER(C.c_float))
    ch = np.array(channels, np.int32)
    cp = ch.ctypes.data_as(C.POINTER(C.c_int32))
    ip = lambda *v: np.array(v, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    cap = 64 * d

    def config(**kw):
        c = capi.ChanConfig(C.sizeof(capi.ChanConfig), m, d, t, capi.DDC_CU8, cap, 0, len(channels))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    h = vp()
    chan = capi.Chan(m, d, taps, channels, in_format=capi.DDC_CU8, max_in_samples=cap)
    chan.set_stream(torch.cuda.current_stream().cuda_stream)
    chan.set_first_sample(8 * d)
    raw_in = torch.zeros((cap + 8, 2), dtype=torch.uint8, device="cuda")
    out = torch.zeros((2, 80, 2), dtype=torch.float32, device="cuda")
    i_ok, o_ok = vp(raw_in.data_ptr()), vp(out.data_ptr())
    create = L.sdr_chan_create
    refusals = [
        (capi.ERR_BAD_ARG, create, C.byref(config(struct_size=28)), tp, cp, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(n_channels=0)), tp, cp, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(n_channels=1, decimation=1, n_taps=16, n_out=1)), tp, None, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(n_channels=6, decimation=6, n_taps=12)), tp, cp, C.byref(h)),   # not a power of two
        (capi.ERR_BAD_ARG, create, C.byref(config(n_channels=512, decimation=512, n_taps=512, max_in_samples=512)), tp, cp, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(decimation=0)), tp, cp, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(decimation=1)), tp, cp, C.byref(h)),                          # M / 8
        (capi.ERR_BAD_ARG, create, C.byref(config(decimation=16, max_in_samples=256)), tp, cp, C.byref(h)),     # 2 M
        (capi.ERR_BAD_ARG, create, C.byref(config(decimation=3, max_in_samples=3 * 64)), tp, cp, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(n_channels=2, decimation=0, n_taps=16)), tp, cp, C.byref(h)),  # M / 4 below 1
        (capi.ERR_BAD_ARG, create, C.byref(config(n_taps=0)), tp, cp, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(n_taps=t + 1)), tp, cp, C.byref(h)),                          # not P M
        (capi.ERR_BAD_ARG, create, C.byref(config(n_taps=65 * m)), tp, cp, C.byref(h)),                         # P above 64
        (capi.ERR_BAD_ARG, create, C.byref(config(n_channels=256, decimation=64, n_taps=4096 + 256)), tp, cp, C.byref(h)),  # T above 4096
        (capi.ERR_BAD_ARG, create, C.byref(config(in_format=4)), tp, cp, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(in_format=-1)), tp, cp, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(max_in_samples=cap + 1)), tp, cp, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(max_in_samples=0)), tp, cp, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(n_out=0)), tp, cp, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config(n_out=m + 1)), tp, None, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config()), None, cp, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config()), tp, cp, None),
        (capi.ERR_BAD_ARG, create, None, tp, cp, C.byref(h)),
        (capi.ERR_BAD_ARG, create, C.byref(config()), tp, ip(5, 5), C.byref(h)),    # not distinct
        (capi.ERR_BAD_ARG, create, C.byref(config()), tp, ip(5, m), C.byref(h)),    # above M - 1
        (capi.ERR_BAD_ARG, create, C.byref(config()), tp, ip(-1, 0), C.byref(h)),
        (capi.ERR_BAD_ARG, L.sdr_chan_process_device, chan._h, vp(raw_in.data_ptr() + 2), 8 * d, o_ok, 8),   # misaligned input
        (capi.ERR_BAD_ARG, L.sdr_chan_process_device, chan._h, i_ok, 8 * d, vp(out.data_ptr() + 8), 8),      # misaligned output
        (capi.ERR_BAD_ARG, L.sdr_chan_process_device, chan._h, None, 8 * d, o_ok, 8),
        (capi.ERR_BAD_ARG, L.sdr_chan_process_device, chan._h, i_ok, 8 * d, None, 8),
        (capi.ERR_BAD_ARG, L.sdr_chan_process_device, None, i_ok, 8 * d, o_ok, 8),
        (capi.ERR_BAD_SIZE, L.sdr_chan_process_device, chan._h, i_ok, 8 * d + 1, o_ok, 12),  # not a multiple of D
        (capi.ERR_BAD_SIZE, L.sdr_chan_process_device, chan._h, i_ok, 0, o_ok, 8),
        (capi.ERR_BAD_SIZE, L.sdr_chan_process_device, chan._h, i_ok, cap + d, o_ok, 80),    # above the capacity
        (capi.ERR_BAD_ARG, L.sdr_chan_process_device, chan._h, i_ok, 8 * d, o_ok, 4),        # a stride below the outputs
        (capi.ERR_BAD_ARG, L.sdr_chan_process_device, chan._h, i_ok, 8 * d, o_ok, 10),       # not a multiple of 4
        (capi.ERR_BAD_SIZE, L.sdr_chan_process_host, chan._h, vp(ch.ctypes.data), d + 1, o_ok, 8),
        (capi.ERR_BAD_ARG, L.sdr_chan_process_host, chan._h, None, 8 * d, o_ok, 8),
        (capi.ERR_STATE, L.sdr_chan_set_first_sample, chan._h, 16 * d),  # (after the first good call, below)
    ]
    assert L.sdr_chan_set_first_sample(chan._h, -d) == capi.ERR_BAD_ARG and L.sdr_chan_set_first_sample(chan._h, 8 * d + 1) == capi.ERR_BAD_ARG
    assert chan.total_samples == 8 * d
    # a good call of 8 outputs in front of the first refusal and behind every one: the stream goes on as if nothing was tried
    piece = 8 * d
    raw = R.random_raw(piece * (len(refusals) + 1), R.CU8, 16)
    want = CR.chan_ref(R.to_f32(raw, R.CU8), m, d, taps, *table, channels=channels, first_sample=8 * d)
    for i in range(len(refusals) + 1):
        if i:
            status, call, *args = refusals[-i]
            h.value = 0xdead
            assert call(*args) == status, (i, L.sdr_last_error())
            assert h.value == 0xdead and L.sdr_last_error()
            assert chan.total_samples == 8 * d + i * piece
        raw_in[:piece] = torch.from_numpy(raw[i * piece:(i + 1) * piece]).cuda()
        chan.process_device(raw_in.data_ptr(), piece, out.data_ptr(), 80)
        chan.sync()
        assert bits_equal(out.cpu().numpy()[:, :8], want[:, 8 * i:8 * i + 8]), f"the good call behind refusal {i}"
    chan.close()


def ragged_lengths(narrow, hop):
    """Call lengths in outputs, drawn with a fixed seed, as a receiver's are: each even (the next call's output pointer
    stays 16-byte aligned), none a multiple of the hop, a third of them shorter than a hop - after which the bank often has
    no whole new frame."""
    rng = np.random.default_rng(20_241)
    lens, left = [], narrow
    while left > 0:
        k = 2 * int(rng.integers(1, hop // 2) if rng.random() < 0.35 else rng.integers(hop, 100 * hop))
        k += 2 * (k % hop == 0)
        lens.append(min(k, left))
        left -= lens[-1]
    assert all(k % 2 == 0 for k in lens) and all(k % hop for k in lens[:-1]) and sum(lens) == narrow
    return lens


@pytest.fixture(scope="module")
def e2e(table):
    """Per shape, computed once: the wide stream, the reference's narrow streams and the oracle receiver's outputs."""
    raw, narrow = CR.e2e_wide()
    e = CR.E2E
    centers = [14_000_000 + int(round(s * e["wide_rate"] / CR.L)) for s in e["steps"]]
    done = {}

    def of(m_key):
        if m_key not in done:
            m, d, channels = CR.SHAPES[m_key]
            ref = CR.chan_ref(R.to_f32(raw, R.CU8), m, d, CR.e2e_taps(), *table, channels=channels)
            _, outs, decs = run_oracle(e["rate"], e["n"], e["edge"], [[b] for b in e["bins"]], list(ref), centers, e["hop"])
            done[m_key] = (ref, outs, decs)
        return (raw, narrow, centers) + done[m_key]

    return of


def chain(capi, e2e, m_key, lens=None):
    """cu8 wide stream -> channelizer -> bank (N = 512, hop 128, sdr_process_device_stream), both on one HIP stream, call
    pairs back to back with no host synchronisation between a pair's two calls and one at the end.  lens: the channelizer
    calls' outputs (by default 512 frames' worth each); the bank takes whatever whole frames exist behind each and is
    skipped where there is none."""
    import torch

    e = CR.E2E
    n, hop, rate, frames = e["n"], e["hop"], e["rate"], e["frames"]
    m, d, channels = CR.SHAPES[m_key]
    raw, narrow, centers, ref, outs, decs = e2e(m_key)
    taps = CR.e2e_taps()
    per = 512  # frames' worth of samples per channelizer call, at the most
    if lens is None:
        lens = [min(per * hop, narrow - a) for a in range(0, narrow, per * hop)]
    assert sum(lens) == narrow and max(lens) <= per * hop
    stride = narrow
    assert stride % 4 == 0
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        wide = torch.from_numpy(raw).cuda()
        out = torch.full((2, stride, 2), float("nan"), dtype=torch.float32, device="cuda")
    stream.synchronize()
    bank = capi.Bank(rate, n, n_bands=2, edge_width=e["edge"], max_batch_frames=per, max_listeners=2, hop=hop)
    chan = capi.Chan(m, d, taps, channels, in_format=capi.DDC_CU8, max_in_samples=per * hop * d)
    bank.set_stream(stream.cuda_stream)
    chan.set_stream(stream.cuda_stream)
    for b in range(2):
        bank.set_center_frequency(b, centers[b])
        assert bank.attach(b, e["bins"][b]) == 0
    bank.enable_results(True)
    have = done = skipped = 0  # narrow samples produced, frames processed, calls behind which the bank had no new frame
    batches = []
    for k in lens:
        chan.process_device(wide.data_ptr() + have * d * 2, k * d, out.data_ptr() + have * 8, stride)
        have += k
        f = (have - n) // hop + 1 - done if have >= n else 0
        if f == 0:
            skipped += 1
            continue
        bank.process_device_stream(out.data_ptr() + done * hop * 8, f, stride)
        batches.append((done, done + f))
        done += f
    chan.sync()
    bank.sync()
    assert have == narrow and done == frames and len(batches) >= 3 and bank.total_frames == frames
    got = out.cpu().numpy()
    assert bits_equal(got, ref)
    text = [[""], [""]]
    n_peaks = 0
    for a, z in batches:
        res = bank.poll(wait=True)
        n_peaks += check_batch_polled(res, outs, a, z, 1, text, 2)[1]
    assert bank.poll() is None
    assert n_peaks > 0 and sum(len(o["peak_frames"]) for o in outs) >= 6  # at least three cumulations per band
    for b, call in enumerate(e["calls"]):
        assert text[b][0] == decs[b][0][0] and call in text[b][0], text[b][0]
    chan.close()
    bank.close()
    return skipped


@pytest.mark.parametrize("m_key", sorted(CR.SHAPES))
def test_end_to_end_with_a_bank_on_one_stream(capi, e2e, m_key):
    """Every channelizer call makes a whole number of hops."""
    assert chain(capi, e2e, m_key) == 0


@pytest.mark.parametrize("m_key", sorted(CR.SHAPES))
def test_end_to_end_with_ragged_calls(capi, e2e, m_key):
    """The same stream cut as a receiver cuts it (ragged_lengths): the same samples, peaks, edges and text."""
    lens = ragged_lengths(CR.e2e_wide()[1], CR.E2E["hop"])
    assert len(lens) >= 8
    assert chain(capi, e2e, m_key, lens) >= 2  # (calls behind which the bank was skipped)
