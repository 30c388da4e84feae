"""The impulse noise blanker on the GPU (sdr_nb_*; csrc/k_nb.hip, capi_nb.hip) against tests/nb_ref.py, byte for byte and
with equal statistics: every format at lengths around the gate kernel's tile, full-scale samples planted where a block, a
tile and a call begin and end and where judging begins, the gate's limits hold = 0 and hold = B, one stream cut into calls
shorter than the window, thresholds changed between calls with a gate open, both entry points, a restart above 2^32, every
refusal with a good call behind it, and one cu8 stream through blanker, DDC and bank on one HIP stream against the oracle
receiver fed ddc_ref(nb_ref(raw)).  Every case here has B = 64 (the chain: 256) and W = 2 or 8; the block sizes up to 4096,
and with them every branch the kernels take on the block's size, W = 1 and 64, holds above 256 samples and above a wave's
4 KB, equality in the inequality and the saturated threshold are covered by the seeded fuzz, tests/test_nb_fuzz_gpu.py."""
import ctypes as C

import numpy as np
import pytest

import ddc_ref as R
import nb_ref as N
from nb_run import run_nb
from parity_tools import bits_equal, capi, check_batch_polled, run_oracle  # noqa: F401
from sdrainer_amd import synth

pytestmark = pytest.mark.gpu

B, W = 64, 2


def quiet(n, fmt, seed):
    """A few LSB of noise around the centre: a full-scale sample is an impulse at any ratio the tests use."""
    return N.random_raw(n, fmt, seed, 100 if (fmt & ~N.REAL) == N.SC16 else 3)


def plant(raw, fmt, places):
    for p in places:
        if 0 <= p < len(raw):
            raw[p] = N.full_scale(fmt)
    return raw


def cut(raw, lens):
    assert sum(lens) == len(raw)
    cuts = np.cumsum([0] + list(lens))
    return [raw[a:e] for a, e in zip(cuts[:-1], cuts[1:])]


def ref_pieces(fmt, block, window, ratio, hold, pieces, thresholds=None, first_sample=0, reads=()):
    ref = N.NbRef(fmt, block, window, ratio, hold, first_sample)
    outs, read = [], []
    for i, p in enumerate(pieces):
        if thresholds is not None and thresholds[i] is not None:
            ref.set_threshold(*thresholds[i])
        outs.append(ref.process(p))
        if i in reads:
            read.append(ref.read_stats())
    read.append(ref.read_stats())
    return outs, read


def check(got, want, what=""):
    outs, reads = got
    wouts, wreads = want
    assert len(outs) == len(wouts)
    for i, (g, w) in enumerate(zip(outs, wouts)):
        assert bits_equal(g, w), f"{what} call {i}: first difference at sample {int(np.flatnonzero((g != w).reshape(len(g), -1).any(axis=1))[0])}"
    assert reads == wreads, what


def lengths(tile, block):
    out = []
    for n in (block, 2 * block, tile - block, tile, tile + block, 2 * tile + 3 * block):
        if n > 0 and n not in out:
            out.append(n)
    return out


# -- formats and lengths, planted impulses ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", N.FORMATS, ids=N.FORMAT_IDS)
def test_every_format_at_lengths_around_a_tile(capi, fmt):
    """Each length three times on one object and a call of one block behind them: the first call warms up, the later
    ones are judged from their first sample on.  Full-scale samples at every call's first and last sample (the gate runs
    into the next call), at a tile's and a block's first and last sample, at the last sample of block W - 1 (not judged)
    and the first of block W (judged)."""
    tile = capi.nb_tile_samples(fmt, B)
    assert tile == 16384 // (N.RAW_DTYPE[fmt]().itemsize * (1 if N.is_real(fmt) else 2))
    hold, ratio = 3, 64
    for n in lengths(tile, B):
        raw = quiet(3 * n + B, fmt, 7 * n + fmt)
        places = [W * B - 1, W * B]
        for o in (0, n, 2 * n, 3 * n):
            places += [o, o - 1, o + 5 * B - 1, o + 5 * B]
            places += [o + t * tile + d for t in (1, 2) for d in (-1, 0) if t * tile <= n]
        plant(raw, fmt, places)
        pieces = cut(raw, [n, n, n, B])
        want = ref_pieces(fmt, B, W, ratio, hold, pieces)
        # (the reference first: block W's first sample is an impulse, block W - 1's last is not, and a gate crosses a call's end)
        whole = np.concatenate(want[0])
        if len(raw) > W * B:
            assert bits_equal(whole[W * B - 1], raw[W * B - 1]) and not bits_equal(whole[W * B], raw[W * B])
        assert bits_equal(whole[2 * n:2 * n + 1 + hold], N.blank_words(np.arange(2 * n, 2 * n + 1 + hold), fmt)) and want[1][0]["impulses"] >= 3
        check(run_nb(capi, fmt, B, W, ratio, hold, pieces), want, f"{n} samples")


@pytest.mark.parametrize("fmt", [N.CU8, N.SC16, N.RS8], ids=["cu8", "sc16", "rs8"])
@pytest.mark.parametrize("hold", [0, B])
def test_gate_limits(capi, fmt, hold):
    """hold = B: the lookback in front of a tile spans a whole block, and a gate opened by a call's last sample covers the
    whole of a next call of one block."""
    tile = capi.nb_tile_samples(fmt, B)
    lens = [tile + B, B, 2 * tile, B, B]
    raw = quiet(sum(lens), fmt, 90 + fmt + hold)
    plant(raw, fmt, [tile - 1, tile + B - 1, tile + 2 * B + tile - B, tile + 2 * B + tile - 1, sum(lens[:3]) - 1, sum(lens[:4]) + 7])
    pieces = cut(raw, lens)
    want = ref_pieces(fmt, B, W, 64, hold, pieces)
    if hold == B:
        assert bits_equal(want[0][1], N.blank_words(np.arange(B) + lens[0], fmt))  # the second call: blank throughout
    check(run_nb(capi, fmt, B, W, 64, hold, pieces), want)


# -- cuts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", N.FORMATS, ids=N.FORMAT_IDS)
def test_any_cut_gives_the_same_bytes_and_statistics(capi, fmt):
    """W = 8: the calls of one block leave old powers in place.  Whole-range random words, so that impulses are frequent."""
    w, hold, ratio = 8, 5, 32
    tile = capi.nb_tile_samples(fmt, B)
    lens = [B, 5 * B, B, B, tile + B]
    for kind in ("wild", "quiet"):
        raw = N.random_raw(sum(lens), fmt, 200 + fmt) if kind == "wild" else plant(quiet(sum(lens), fmt, 300 + fmt), fmt, [8 * B - 1, 8 * B, 9 * B + 3, 9 * B + 5, 20 * B])
        want, wstats = N.nb_ref(raw, fmt, B, w, ratio, hold)
        assert wstats["impulses"] > 0 and wstats["blanked"] > wstats["impulses"]
        (whole,), (one,) = run_nb(capi, fmt, B, w, ratio, hold, [raw])
        outs, reads = run_nb(capi, fmt, B, w, ratio, hold, cut(raw, lens), reads=(1, 3))
        assert bits_equal(whole, want) and one == wstats, kind
        assert bits_equal(np.concatenate(outs), want), kind
        total = reads[0]
        for r in reads[1:]:
            total = N.add_stats(total, r)
        assert len(reads) == 3 and total == wstats, kind


# -- thresholds changed between calls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [N.CS8, N.RU8, N.SC16], ids=["cs8", "ru8", "sc16"])
def test_threshold_changes_between_calls(capi, fmt):
    """Off, on, a shorter hold while a long gate is open (it keeps its length), a higher ratio, off with a gate open, on."""
    lens = [4 * B, 2 * B, 2 * B, 3 * B, 2 * B, 2 * B, 2 * B]
    thresholds = [None, (64, 40), (64, 1), (16384, 1), (0, 9), None, (32, B)]
    raw = quiet(sum(lens), fmt, 400 + fmt)
    ends = np.cumsum(lens)
    plant(raw, fmt, [3 * B, ends[1] - 1, ends[1] + 10, ends[2] - 1, ends[3] - 1, ends[4] + 3, ends[5] + 1, ends[6] - 1])
    pieces = cut(raw, lens)
    want = ref_pieces(fmt, B, W, 0, 9, pieces, thresholds)
    # the reference: nothing while off; the gate of 40 opened by call 1's last sample runs 40 samples into call 2
    assert bits_equal(want[0][0], pieces[0]) and bits_equal(want[0][5], pieces[5])
    assert bits_equal(want[0][2][:40], N.blank_words(np.arange(40) + ends[1], fmt)) and bits_equal(want[0][2][40], pieces[2][40])
    assert bits_equal(want[0][4][:1], N.blank_words(ends[3:4], fmt)) and bits_equal(want[0][4][1:], pieces[4][1:])
    check(run_nb(capi, fmt, B, W, 0, 9, pieces, thresholds=thresholds), want)


# -- entry points -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", N.FORMATS, ids=N.FORMAT_IDS)
def test_process_host_equals_process_device(capi, fmt):
    tile = capi.nb_tile_samples(fmt, B)
    lens = [3 * B, B, tile + 2 * B, B]
    raw = N.random_raw(sum(lens), fmt, 500 + fmt)
    pieces = cut(raw, lens)
    want = ref_pieces(fmt, B, W, 32, 2, pieces)
    assert want[1][0]["impulses"] > 0
    check(run_nb(capi, fmt, B, W, 32, 2, pieces, host=True), want, "host")
    check(run_nb(capi, fmt, B, W, 32, 2, pieces, host=[False, True, False, True]), want, "mixed")


# -- restart ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [N.CU8, N.RU8], ids=["cu8", "ru8"])
def test_restart_at_a_large_first_sample(capi, fmt):
    """k0 an odd number of blocks above 2^32: the warm-up starts again, and the uint8 blank word's parity is the absolute
    k's (k0 is even, so it is also the call's)."""
    k0 = ((1 << 32) // B + 12_345) * B
    assert (k0 // B) % 2 == 1 and k0 > 1 << 32
    lens = [B, 3 * B, 2 * B]
    raw = plant(quiet(sum(lens), fmt, 600 + fmt), fmt, [B + 1, 2 * B + 1, 2 * B + 4, 4 * B - 1])
    pieces = cut(raw, lens)
    want = ref_pieces(fmt, B, W, 64, 2, pieces, first_sample=k0)
    whole = np.concatenate(want[0])
    assert bits_equal(whole[:2 * B], raw[:2 * B])  # block 1's sample is not judged: W = 2 blocks warm up
    assert bits_equal(whole[2 * B + 1:2 * B + 4], N.blank_words(np.arange(2 * B + 1, 2 * B + 4), fmt))
    check(run_nb(capi, fmt, B, W, 64, 2, pieces, first_sample=k0), want)


# -- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(capi):
    """A good call behind every refusal: its bytes, sdr_nb_total_samples and the statistics show that nothing moved."""
    import torch

    L = capi.load()
    vp = C.c_void_p
    fmt, hold, ratio = N.CU8, 3, 64
    cap = 4 * B
    stream = torch.cuda.current_stream().cuda_stream

    def cfg(**kw):
        f = dict(struct_size=C.sizeof(capi.NbConfig), in_format=fmt, block=B, window=W, ratio_q4=ratio, hold=hold, max_in_samples=cap, device_id=0)
        f.update(kw)
        return C.byref(capi.NbConfig(*[f[k] for k, _ in capi.NbConfig._fields_]))

    h = vp()
    for bad in (dict(struct_size=28), dict(in_format=capi.DDC_F32), dict(in_format=capi.DDC_RF32), dict(in_format=4), dict(block=32),
                dict(block=96), dict(block=8192), dict(window=0), dict(window=3), dict(window=128), dict(block=4096, window=32),
                dict(ratio_q4=15), dict(ratio_q4=16385), dict(ratio_q4=-1), dict(hold=-1), dict(hold=B + 1), dict(max_in_samples=0),
                dict(max_in_samples=B + 1)):
        assert L.sdr_nb_create(cfg(**bad), C.byref(h)) == capi.ERR_BAD_ARG and not h.value, bad
    assert L.sdr_nb_create(None, C.byref(h)) == capi.ERR_BAD_ARG and L.sdr_nb_create(cfg(), None) == capi.ERR_BAD_ARG
    assert capi.nb_tile_samples(capi.DDC_F32, B) < 0 and capi.nb_tile_samples(fmt, 100) < 0

    nb = capi.Nb(fmt, B, W, ratio, hold, max_in_samples=cap)
    nb.set_stream(stream)
    buf = torch.zeros((2 * cap + 16, 2), dtype=torch.uint8, device="cuda")
    out = torch.zeros((cap + 8, 2), dtype=torch.uint8, device="cuda")
    i_ok, o_ok = vp(buf.data_ptr()), vp(out.data_ptr())
    stats = capi.NbStats()
    host_in = np.zeros((cap, 2), np.uint8)
    refusals = [
        (capi.ERR_BAD_ARG, L.sdr_nb_process_device, None, i_ok, B, o_ok),
        (capi.ERR_BAD_ARG, L.sdr_nb_process_device, nb._h, None, B, o_ok),
        (capi.ERR_BAD_ARG, L.sdr_nb_process_device, nb._h, i_ok, B, None),
        (capi.ERR_BAD_SIZE, L.sdr_nb_process_device, nb._h, i_ok, 0, o_ok),
        (capi.ERR_BAD_SIZE, L.sdr_nb_process_device, nb._h, i_ok, B + 1, o_ok),
        (capi.ERR_BAD_SIZE, L.sdr_nb_process_device, nb._h, i_ok, B // 2, o_ok),
        (capi.ERR_BAD_SIZE, L.sdr_nb_process_device, nb._h, i_ok, cap + B, o_ok),
        (capi.ERR_BAD_ARG, L.sdr_nb_process_device, nb._h, vp(buf.data_ptr() + 2), B, o_ok),
        (capi.ERR_BAD_ARG, L.sdr_nb_process_device, nb._h, i_ok, B, vp(out.data_ptr() + 8)),
        (capi.ERR_BAD_ARG, L.sdr_nb_process_device, nb._h, i_ok, 2 * B, i_ok),  # in place
        (capi.ERR_BAD_ARG, L.sdr_nb_process_device, nb._h, i_ok, 2 * B, vp(buf.data_ptr() + 2 * B)),  # the ranges overlap
        (capi.ERR_BAD_ARG, L.sdr_nb_process_device, nb._h, vp(buf.data_ptr() + 2 * B), 2 * B, i_ok),
        (capi.ERR_BAD_ARG, L.sdr_nb_process_host, nb._h, None, B, o_ok),
        (capi.ERR_BAD_SIZE, L.sdr_nb_process_host, nb._h, vp(host_in.ctypes.data), B - 1, o_ok),
        (capi.ERR_BAD_ARG, L.sdr_nb_process_host, nb._h, vp(host_in.ctypes.data), B, vp(out.data_ptr() + 4)),
        (capi.ERR_BAD_ARG, L.sdr_nb_set_threshold, None, 64, 3),
        (capi.ERR_BAD_ARG, L.sdr_nb_set_threshold, nb._h, 8, 3),
        (capi.ERR_BAD_ARG, L.sdr_nb_set_threshold, nb._h, 20000, 3),
        (capi.ERR_BAD_ARG, L.sdr_nb_set_threshold, nb._h, 64, B + 1),
        (capi.ERR_BAD_ARG, L.sdr_nb_set_threshold, nb._h, 64, -1),
        (capi.ERR_STATE, L.sdr_nb_set_first_sample, nb._h, 2 * B),
        (capi.ERR_BAD_ARG, L.sdr_nb_set_first_sample, None, 0),
        (capi.ERR_BAD_ARG, L.sdr_nb_set_stream, None, None),
        (capi.ERR_BAD_ARG, L.sdr_nb_sync, None),
        (capi.ERR_BAD_ARG, L.sdr_nb_read_stats, None, C.byref(stats)),
        (capi.ERR_BAD_ARG, L.sdr_nb_read_stats, nb._h, None),
    ]
    # before the first call: a first sample that is negative or no multiple of B is refused, and the start stays 0
    assert L.sdr_nb_set_first_sample(nb._h, -B) == capi.ERR_BAD_ARG and L.sdr_nb_set_first_sample(nb._h, B + 1) == capi.ERR_BAD_ARG
    assert nb.total_samples == 0 and L.sdr_nb_total_samples(None) == 0
    piece = 2 * B
    raw = quiet(piece * (len(refusals) + 1), fmt, 700)
    plant(raw, fmt, [piece * i + d for i in range(1, len(refusals) + 1) for d in (0, 70, piece - 1)])
    ref = N.NbRef(fmt, B, W, ratio, hold)
    for i in range(len(refusals) + 1):
        if i:
            status, call, *args = refusals[i - 1]
            assert call(*args) == status, (i, L.sdr_last_error())
            assert L.sdr_last_error() and not any(stats.asdict().values())
            assert nb.total_samples == i * piece
        buf[:piece] = torch.from_numpy(raw[i * piece:(i + 1) * piece]).cuda()
        nb.process_device(buf.data_ptr(), piece, out.data_ptr())
        nb.sync()
        assert bits_equal(out.cpu().numpy()[:piece], ref.process(raw[i * piece:(i + 1) * piece])), f"the good call behind refusal {i}"
    want = ref.read_stats()
    assert nb.read_stats() == want and want["impulses"] >= len(refusals)
    nb.close()
    assert L.sdr_nb_destroy(None) == capi.OK


# -- the chain --------------------------------------------------------------------------------------------------------------
CHAIN = dict(R.E2E, steps=(9000,), bins=(320,), texts=("dl1abc dl1abc",), dit_ticks=(8,), frames=1460, sigma=0.1, pulses=300, block=256, window=8, hold=3, ratio=192)


def chain_wide():
    """One keyed carrier and noise as tests/ddc_ref.py's fixture builds them, cu8, with samples (255, 0) planted at random
    places behind the blanker's warm-up."""
    e = CHAIN
    narrow = (e["frames"] - 1) * e["hop"] + e["n"]
    wide = narrow * e["decimation"]
    offset = e["steps"][0] * e["wide_rate"] / R.L + (e["bins"][0] - e["n"] // 2) * e["rate"] / e["n"]
    key = np.repeat(np.concatenate([np.zeros(40, np.uint8), synth.keying_pattern(e["texts"][0], e["dit_ticks"][0])]), e["hop"] * e["decimation"])
    raw = synth.wide_stream(wide, e["wide_rate"], [(offset, e["amplitude"], key)], noise_sigma=e["sigma"], seed=e["seed"], quantise="cu8")
    places = np.sort(np.random.default_rng(5).choice(np.arange(e["window"] * e["block"], wide), e["pulses"], replace=False))
    raw[places] = (255, 0)
    return raw, narrow, places


def test_chain_blanker_ddc_bank_on_one_stream(capi):
    import torch

    e = CHAIN
    n, hop, rate, d, frames = e["n"], e["hop"], e["rate"], e["decimation"], e["frames"]
    table = capi.ddc_nco_table()
    raw, narrow, places = chain_wide()
    assert narrow * d == len(raw) and len(raw) % e["block"] == 0
    blanked, stats = N.nb_ref(raw, N.CU8, e["block"], e["window"], e["ratio"], e["hold"])
    assert stats["impulses"] >= e["pulses"] // 2 and not np.array_equal(blanked, raw)
    taps = R.e2e_taps()
    ref = R.ddc_ref(R.to_f32(blanked, R.CU8), d, taps, e["steps"], *table)
    center = [14_000_000 + int(round(e["steps"][0] * e["wide_rate"] / R.L))]
    _, outs, decs = run_oracle(rate, n, e["edge"], [[e["bins"][0]]], list(ref), center, hop)
    assert e["calls"][0] in decs[0][0][0], decs[0][0][0]
    per = 256
    lens = [min(per * hop, narrow - a) for a in range(0, narrow, per * hop)]
    assert all((m * d) % e["block"] == 0 for m in lens)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        wide = torch.from_numpy(raw).cuda()
        clean = torch.full((per * hop * d + 32, 2), 0xA5, dtype=torch.uint8, device="cuda")
        out = torch.full((1, narrow, 2), float("nan"), dtype=torch.float32, device="cuda")
    stream.synchronize()
    bank = capi.Bank(rate, n, n_bands=1, edge_width=e["edge"], max_batch_frames=per + 4, max_listeners=2, hop=hop)
    ddc = capi.Ddc(d, taps, e["steps"], in_format=capi.DDC_CU8, max_in_samples=per * hop * d)
    nb = capi.Nb(capi.DDC_CU8, e["block"], e["window"], e["ratio"], e["hold"], max_in_samples=per * hop * d)
    for o in (bank, ddc, nb):
        o.set_stream(stream.cuda_stream)
    bank.set_center_frequency(0, center[0])
    assert bank.attach(0, e["bins"][0]) == 0
    bank.enable_results(True)
    have = done = 0
    batches = []
    for m in lens:
        nb.process_device(wide.data_ptr() + have * d * 2, m * d, clean.data_ptr())
        ddc.process_device(clean.data_ptr(), m * d, out.data_ptr() + have * 8, narrow)
        have += m
        k = (have - n) // hop + 1 - done if have >= n else 0
        if k == 0:
            continue
        bank.process_device_stream(out.data_ptr() + done * hop * 8, k, narrow)
        batches.append((done, done + k))
        done += k
    bank.sync()
    assert nb.read_stats() == stats
    assert have == narrow and done == frames and len(batches) >= 3 and bank.total_frames == frames
    assert bits_equal(out.cpu().numpy(), ref)
    text = [[""]]
    n_peaks = 0
    for a, z in batches:
        n_peaks += check_batch_polled(bank.poll(wait=True), outs, a, z, 1, text, 1, live=[[0]])[1]
    assert bank.poll() is None and n_peaks > 0
    assert text[0][0] == decs[0][0][0] and e["calls"][0] in text[0][0]
    for o in (nb, ddc, bank):
        o.close()
