"""The IQ correction and the raw stream's sums on the GPU (sdr_iq_*_set_correction, sdr_iq_*_enable_sums, sdr_iq_*_read_sums;
csrc/k_ddc_iqc.hip, k_chan_iqc.hip, k_iq_sums.hip) against tests/iqc_ref.py, bit for bit: a corrected DDC and channelizer are
tests/ddc_ref.py and tests/chan_ref.py fed the corrected float32 values - every complex format, output counts around a
tile, cuts of the stream into calls, a correction changed and removed between calls, float32 specials across the carry -
the sums are the int64 sums of the raw words for any cut and either entry point, every refusal changes nothing, and the
impaired cu8 fixture goes through sums, sdr_iq_correction_from_sums, a corrected DDC and a three-band bank on one HIP
stream, against the oracle receiver fed the corrected reference streams."""
import ctypes as C

import numpy as np
import pytest

import chan_ref as CR
import ddc_real as RR
import ddc_ref as R
import iqc_ref as Q
from iqc_run import KEEP, run_chan, run_ddc
from parity_tools import bits_equal, capi, check_batch_polled, nan_equal_bits  # noqa: F401

pytestmark = pytest.mark.gpu

STEPS = (9000, -32768)  # two bands
CORR = (0.0123, -0.0217, 1.0471, -0.0533)  # all four fields non-trivial
CORR2 = (-0.3, 0.002, 0.87, 0.11)
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** 100, 2.0 ** -100, 1e-40, -1e-42], np.float32)


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


def random_taps(t, seed):
    return np.random.default_rng(seed).uniform(-1, 1, t).astype(np.float32)


def cut(raw, lens):
    assert sum(lens) == len(raw)
    cuts = np.cumsum([0] + list(lens))
    return [raw[a:e] for a, e in zip(cuts[:-1], cuts[1:])]


# -- the corrected down-converter -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.FORMATS, ids=R.FORMAT_IDS)
@pytest.mark.parametrize("d,t", [(8, 64), (3, 7), (1, 1)])
def test_corrected_ddc_equals_the_reference(capi, table, fmt, d, t):
    tile = capi.DDC_TILE_OUTPUTS
    assert tile == 512
    counts = (1, tile - 1, tile, tile + 1, 2 * tile + 37)
    taps = random_taps(t, 100 * d + t)
    raw = R.random_raw(d * max(counts), fmt, 7 * d + t + fmt)
    want = R.ddc_ref(Q.correct(R.to_f32(raw, fmt), CORR), d, taps, STEPS, *table)
    plain = R.ddc_ref(R.to_f32(raw, fmt), d, taps, STEPS, *table)
    assert not bits_equal(want, plain)
    for m in counts:
        got, _ = run_ddc(capi, fmt, d, taps, STEPS, [raw[:m * d]], corrs=[CORR])
        assert got.shape == (len(STEPS), m, 2)
        assert bits_equal(got, want[:, :m]), f"{m} outputs"


@pytest.mark.parametrize("fmt", R.FORMATS, ids=R.FORMAT_IDS)
@pytest.mark.parametrize("d,t", [(8, 64), (3, 7)])
def test_corrected_ddc_call_cuts(capi, table, fmt, d, t):
    """Calls of D and 5 D samples, two consecutive calls shorter than T - 1 (part of the carry survives each), the rest."""
    taps = random_taps(t, 5)
    short = (t - 1) // d // 2 * d
    assert 0 < short < t - 1
    lens = [d, 5 * d, short, short, 700 * d]
    raw = R.random_raw(sum(lens), fmt, 900 + fmt)
    want = R.ddc_ref(Q.correct(R.to_f32(raw, fmt), CORR), d, taps, STEPS, *table)
    whole, _ = run_ddc(capi, fmt, d, taps, STEPS, [raw], corrs=[CORR])
    pieces, _ = run_ddc(capi, fmt, d, taps, STEPS, cut(raw, lens), corrs=[CORR] + [KEEP] * 4)
    assert bits_equal(whole, want) and bits_equal(pieces, want)


@pytest.mark.parametrize("fmt", [R.F32, R.CU8, R.SC16], ids=["f32", "cu8", "sc16"])
def test_correction_changed_and_removed_between_calls(capi, table, fmt):
    """None at first, set, changed (behind a call shorter than T - 1), removed with NULL: the carried RAW samples are read
    again with each call's values.  Behind NULL the bits are an uncorrected DDC's."""
    d, t = 8, 64
    taps = random_taps(t, 12)
    lens = [70 * d, 64 * d, 3 * d, 200 * d, 5 * d, 90 * d]
    corrs = [KEEP, CORR, CORR2, KEEP, None, KEEP]
    current = [None, CORR, CORR2, CORR2, None, None]
    raw = R.random_raw(sum(lens), fmt, 32 + fmt)
    pieces = cut(raw, lens)
    ref = Q.CorrectedDdcRef(d, taps, STEPS, *table)
    want = np.concatenate([ref.process(R.to_f32(p, fmt), c) for p, c in zip(pieces, current)], axis=1)
    got, _ = run_ddc(capi, fmt, d, taps, STEPS, pieces, corrs=corrs)
    assert bits_equal(got, want)
    plain = R.ddc_ref(R.to_f32(raw, fmt), d, taps, STEPS, *table)
    first, last = lens[0] // d, sum(lens[:4]) // d
    assert bits_equal(got[:, :first], plain[:, :first]) and bits_equal(got[:, last:], plain[:, last:])
    assert not bits_equal(got[:, first:last], plain[:, first:last])


def with_specials(n, places, seed):
    """float32 [n, 2] in [-1, 1) with SPECIALS at consecutive samples from each place on: in I, and three samples later in Q."""
    x = R.random_raw(n, R.F32, seed)
    for p in places:
        x[p:p + len(SPECIALS), 0] = SPECIALS
        x[p + 3:p + 3 + len(SPECIALS), 1] = SPECIALS
    return x


def test_float32_specials_in_every_position_of_a_group(capi, table):
    """+-0, +-Inf, NaN, 2^+-100 and subnormals, nine consecutive samples each time (every position of a 16-byte group), once
    inside a call and once across the cut between two calls, where part of the run is read from the carry."""
    d, t = 3, 7
    taps = random_taps(t, 21)
    lens = [40 * d, 2 * d, 60 * d]
    x = with_specials(sum(lens), [17, lens[0] - 4, lens[0] + lens[1] - 5], 23)
    with np.errstate(all="ignore"):
        want = R.ddc_ref(Q.correct(x, CORR), d, taps, STEPS, *table)
    got, _ = run_ddc(capi, R.F32, d, taps, STEPS, cut(x, lens), corrs=[CORR, KEEP, KEEP])
    assert nan_equal_bits(got, want)
    assert np.isnan(want).any() and np.isfinite(want).sum() > want.size // 2  # (an Inf sample is NaN behind the mix)
    m, dd, p = 8, 4, 4
    ctaps = random_taps(m * p, 22)
    lens = [40 * dd, 2 * dd, 60 * dd]
    x = with_specials(sum(lens), [18, lens[0] - 4, lens[0] + lens[1] - 5], 24)
    with np.errstate(all="ignore"):
        want = CR.chan_ref(Q.correct(x, CORR), m, dd, ctaps, *table)
    got, _ = run_chan(capi, R.F32, m, dd, ctaps, cut(x, lens), corrs=[CORR, KEEP, KEEP])
    assert nan_equal_bits(got, want)
    assert np.isnan(want).any() and np.isfinite(want).sum() > want.size // 4


# -- the corrected channelizer ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", R.FORMATS, ids=R.FORMAT_IDS)
@pytest.mark.parametrize("m,d,p,channels", [(8, 4, 4, (1, 6, 0)), (16, 4, 3, (15, 0, 5, 8))])
def test_corrected_channelizer_equals_the_reference(capi, table, fmt, m, d, p, channels):
    tile = capi.chan_tile_outputs(m, d, m * p)
    assert tile == 4096 // m
    taps = random_taps(m * p, 40 + m)
    raw = R.random_raw(d * (tile + 1), fmt, 50 + m + fmt)
    want = CR.chan_ref(Q.correct(R.to_f32(raw, fmt), CORR), m, d, taps, *table, channels=channels)
    assert not bits_equal(want, CR.chan_ref(R.to_f32(raw, fmt), m, d, taps, *table, channels=channels))
    for k in (tile - 1, tile, tile + 1):
        got, _ = run_chan(capi, fmt, m, d, taps, [raw[:k * d]], channels=channels, corrs=[CORR])
        assert bits_equal(got, want[:, :k]), f"{k} outputs"
    # cut into calls, the correction removed behind the second: the last call is an uncorrected channelizer's
    lens = [d, 5 * d, (tile - 10) * d, 4 * d]
    got, _ = run_chan(capi, fmt, m, d, taps, cut(raw[:sum(lens)], lens), channels=channels, corrs=[CORR, KEEP, KEEP, None])
    plain = CR.chan_ref(R.to_f32(raw, fmt), m, d, taps, *table, channels=channels)
    a = tile - 4
    assert bits_equal(got[:, :a], want[:, :a]) and bits_equal(got[:, a:], plain[:, a:tile])


# -- the sums ---------------------------------------------------------------------------------------------------------------
def extreme_raw(n, fmt, seed):
    """Only the format's two extreme words, drawn independently for I and Q, with a run of the most negative in front."""
    info = np.iinfo(R.RAW_DTYPE[fmt])
    raw = np.where(np.random.default_rng(seed).random((n, 2)) < 0.5, info.min, info.max).astype(R.RAW_DTYPE[fmt])
    raw[:n // 3] = info.min
    return raw


@pytest.mark.parametrize("fmt", Q.SUM_FORMATS, ids=Q.SUM_FORMAT_IDS)
@pytest.mark.parametrize("kind", ["random", "extreme"])
def test_sums_are_exact_for_any_cut_and_entry_point(capi, table, fmt, kind):
    """D = 3: no call is a whole number of 16-byte groups; 120 003 samples are more than one workgroup's share (32 768
    8-bit, 16 384 sc16 samples) and leave a ragged end of three.  The same totals for one call, for seven, through
    process_host, and with a correction set; the outputs stay the corrected DDC's."""
    d, t = 3, 7
    n = 3 * 40_001
    taps = random_taps(t, 60)
    raw = R.random_raw(n, fmt, 61 + fmt) if kind == "random" else extreme_raw(n, fmt, 62 + fmt)
    want = Q.sums(raw, fmt)
    out1, (one,) = run_ddc(capi, fmt, d, taps, STEPS, [raw], sums=True)
    assert one == want
    lens = [d, 2 * d, 5 * d, 10_922 * d + 3, 16_385 * d - 3, 11 * d]
    lens.append(n - sum(lens))
    assert all(ln % d == 0 for ln in lens) and lens[-1] > 0
    out2, reads = run_ddc(capi, fmt, d, taps, STEPS, cut(raw, lens), sums=True, host=[False, True, False, True, False, True, False],
                          corrs=[KEEP, KEEP, CORR, KEEP, KEEP, KEEP, KEEP], reads=(1, 4))
    assert len(reads) == 3
    total = reads[0]
    for r in reads[1:]:
        total = Q.add_sums(total, r)
    assert total == want
    assert reads[0] == Q.sums(raw[:3 * d], fmt) and reads[1] == Q.sums(raw[3 * d:sum(lens[:5])], fmt)
    assert bits_equal(out1, R.ddc_ref(R.to_f32(raw, fmt), d, taps, STEPS, *table))
    ref = Q.CorrectedDdcRef(d, taps, STEPS, *table)
    cur = [None, None] + [CORR] * 5
    assert bits_equal(out2, np.concatenate([ref.process(R.to_f32(p, fmt), c) for p, c in zip(cut(raw, lens), cur)], axis=1))


@pytest.mark.parametrize("fmt", Q.SUM_FORMATS, ids=Q.SUM_FORMAT_IDS)
def test_channelizer_sums_and_switching_off_and_on(capi, table, fmt):
    import torch

    m, d, p = 8, 2, 4
    taps = random_taps(m * p, 70)
    raw = R.random_raw(d * 2500 + d, fmt, 71 + fmt)
    lens = [d * 2500, d]
    got, (s,) = run_chan(capi, fmt, m, d, taps, cut(raw, lens), sums=True, host=[True, False])
    assert s == Q.sums(raw, fmt)
    assert bits_equal(got, CR.chan_ref(R.to_f32(raw, fmt), m, d, taps, *table))
    # off / on clears; off in a new object; a read while off is refused and clears nothing that a later read would return
    chan = capi.Chan(m, d, taps, None, in_format=fmt, max_in_samples=len(raw))
    chan.set_stream(torch.cuda.current_stream().cuda_stream)
    out = torch.zeros((m, 2504, 2), dtype=torch.float32, device="cuda")
    dev = torch.from_numpy(raw).cuda()
    L = capi.load()
    blank = capi.IqSums()
    assert L.sdr_iq_chan_read_sums(chan._h, C.byref(blank)) == capi.ERR_STATE
    chan.process_device(dev.data_ptr(), lens[0], out.data_ptr(), 2504)  # (not summed: the sums are off)
    chan.enable_iq_sums(True)
    chan.process_device(dev.data_ptr(), 4 * d, out.data_ptr(), 2504)
    chan.enable_iq_sums(False)
    assert L.sdr_iq_chan_read_sums(chan._h, C.byref(blank)) == capi.ERR_STATE and not any(blank.asdict().values())
    chan.enable_iq_sums(True)
    chan.process_device(dev.data_ptr(), 6 * d, out.data_ptr(), 2504)
    assert chan.read_iq_sums() == Q.sums(raw[:6 * d], fmt)
    chan.process_device(dev.data_ptr(), 2 * d, out.data_ptr(), 2504)
    chan.enable_iq_sums(True)  # on while on clears as well
    assert not any(chan.read_iq_sums().values())
    chan.close()


# -- refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing(capi, table):
    """The pattern of tests/test_ddc_gpu.py: a good call behind every refusal, whose outputs and sums show that nothing moved."""
    import torch

    L = capi.load()
    vp = C.c_void_p
    d, t, steps = 4, 16, (100, -200)
    taps = random_taps(t, 15)
    cap = 64 * d
    stream = torch.cuda.current_stream().cuda_stream

    def corr(*v):
        return C.byref(capi.IqCorrection(*v))

    ddc = capi.Ddc(d, taps, steps, in_format=capi.DDC_CU8, max_in_samples=cap)
    chan = capi.Chan(8, 4, random_taps(32, 16), None, in_format=capi.DDC_CU8, max_in_samples=cap)
    f32 = capi.Ddc(d, taps, steps, in_format=capi.DDC_F32, max_in_samples=cap)
    real = capi.Ddc(d, taps, steps, in_format=capi.DDC_RU8, max_in_samples=cap)
    fchan = capi.Chan(8, 4, random_taps(32, 16), None, in_format=capi.DDC_F32, max_in_samples=cap)
    rchan = capi.Chan(8, 4, random_taps(32, 16), None, in_format=capi.DDC_RS16, max_in_samples=cap)
    for o in (ddc, chan, f32, real, fchan, rchan):
        o.set_stream(stream)
    ddc.set_iq_correction(CORR)
    ddc.enable_iq_sums(True)
    chan.set_iq_correction(CORR)
    chan.enable_iq_sums(True)
    raw_in = torch.zeros((cap + 8, 2), dtype=torch.uint8, device="cuda")
    out = torch.zeros((2, 80, 2), dtype=torch.float32, device="cuda")
    cout = torch.zeros((8, 80, 2), dtype=torch.float32, device="cuda")
    i_ok, o_ok = vp(raw_in.data_ptr()), vp(out.data_ptr())
    sums = capi.IqSums()
    nan, inf = float("nan"), float("inf")
    refusals = [
        (capi.ERR_BAD_ARG, L.sdr_iq_ddc_set_correction, None, corr(0, 0, 1, 0)),
        (capi.ERR_BAD_ARG, L.sdr_iq_ddc_set_correction, ddc._h, corr(nan, 0, 1, 0)),
        (capi.ERR_BAD_ARG, L.sdr_iq_ddc_set_correction, ddc._h, corr(0, inf, 1, 0)),
        (capi.ERR_BAD_ARG, L.sdr_iq_ddc_set_correction, ddc._h, corr(0, 0, -inf, 0)),
        (capi.ERR_BAD_ARG, L.sdr_iq_ddc_set_correction, ddc._h, corr(0, 0, 1, nan)),
        (capi.ERR_BAD_ARG, L.sdr_iq_ddc_set_correction, real._h, corr(0, 0, 1, 0)),
        (capi.ERR_BAD_ARG, L.sdr_iq_ddc_set_correction, real._h, None),
        (capi.ERR_BAD_ARG, L.sdr_iq_ddc_enable_sums, None, 1),
        (capi.ERR_BAD_ARG, L.sdr_iq_ddc_enable_sums, f32._h, 1),
        (capi.ERR_BAD_ARG, L.sdr_iq_ddc_enable_sums, real._h, 1),
        (capi.ERR_BAD_ARG, L.sdr_iq_ddc_enable_sums, f32._h, 0),
        (capi.ERR_BAD_ARG, L.sdr_iq_ddc_read_sums, None, C.byref(sums)),
        (capi.ERR_BAD_ARG, L.sdr_iq_ddc_read_sums, ddc._h, None),
        (capi.ERR_STATE, L.sdr_iq_ddc_read_sums, f32._h, C.byref(sums)),
        (capi.ERR_BAD_SIZE, L.sdr_ddc_process_device, ddc._h, i_ok, 8 * d + 1, o_ok, 12),  # (a refused call is not summed)
        (capi.ERR_BAD_ARG, L.sdr_ddc_process_device, ddc._h, vp(raw_in.data_ptr() + 2), 8 * d, o_ok, 8),
        (capi.ERR_BAD_ARG, L.sdr_iq_chan_set_correction, None, corr(0, 0, 1, 0)),
        (capi.ERR_BAD_ARG, L.sdr_iq_chan_set_correction, chan._h, corr(0, 0, nan, 0)),
        (capi.ERR_BAD_ARG, L.sdr_iq_chan_set_correction, chan._h, corr(-inf, 0, 1, 0)),
        (capi.ERR_BAD_ARG, L.sdr_iq_chan_set_correction, rchan._h, corr(0, 0, 1, 0)),
        (capi.ERR_BAD_ARG, L.sdr_iq_chan_enable_sums, None, 1),
        (capi.ERR_BAD_ARG, L.sdr_iq_chan_enable_sums, fchan._h, 1),
        (capi.ERR_BAD_ARG, L.sdr_iq_chan_enable_sums, rchan._h, 1),
        (capi.ERR_BAD_ARG, L.sdr_iq_chan_read_sums, None, C.byref(sums)),
        (capi.ERR_BAD_ARG, L.sdr_iq_chan_read_sums, chan._h, None),
        (capi.ERR_STATE, L.sdr_iq_chan_read_sums, fchan._h, C.byref(sums)),
        (capi.ERR_BAD_SIZE, L.sdr_chan_process_device, chan._h, i_ok, 8 * d + 1, vp(cout.data_ptr()), 12),
    ]
    piece = 8 * d
    raw = R.random_raw(piece * (len(refusals) + 1), R.CU8, 16)
    x = Q.correct(R.to_f32(raw, R.CU8), CORR)
    want = R.ddc_ref(x, d, taps, steps, *table)
    cwant = CR.chan_ref(x, 8, 4, random_taps(32, 16), *table)
    for i in range(len(refusals) + 1):
        if i:
            status, call, *args = refusals[-i]
            assert call(*args) == status, (i, L.sdr_last_error())
            assert L.sdr_last_error() and not any(sums.asdict().values())
            assert ddc.total_samples == chan.total_samples == i * piece
        raw_in[:piece] = torch.from_numpy(raw[i * piece:(i + 1) * piece]).cuda()
        ddc.process_device(raw_in.data_ptr(), piece, out.data_ptr(), 80)
        chan.process_device(raw_in.data_ptr(), piece, cout.data_ptr(), 80)
        ddc.sync()
        chan.sync()
        assert bits_equal(out.cpu().numpy()[:, :8], want[:, 8 * i:8 * i + 8]), f"the DDC's good call behind refusal {i}"
        assert bits_equal(cout.cpu().numpy()[:, :8], cwant[:, 8 * i:8 * i + 8]), f"the channelizer's good call behind refusal {i}"
    assert ddc.read_iq_sums() == Q.sums(raw, R.CU8) and chan.read_iq_sums() == Q.sums(raw, R.CU8)
    # the objects that refused go on as they were: a real DDC without a correction, a float32 one that takes one
    rraw = RR.random_raw_real(piece, RR.RU8, 17)
    real.process_host(rraw, out.data_ptr(), 80)
    real.sync()
    assert bits_equal(out.cpu().numpy()[:, :8], R.ddc_ref(RR.as_complex(RR.to_f32_real(rraw, RR.RU8)), d, taps, steps, *table))
    fraw = R.random_raw(piece, R.F32, 18)
    f32.set_iq_correction(CORR2)
    f32.process_host(fraw, out.data_ptr(), 80)
    f32.sync()
    assert bits_equal(out.cpu().numpy()[:, :8], R.ddc_ref(Q.correct(fraw, CORR2), d, taps, steps, *table))
    for o in (ddc, chan, f32, real, fchan, rchan):
        o.close()


# -- the chain --------------------------------------------------------------------------------------------------------------
def ragged_lengths(narrow, hop):
    """DDC call lengths in outputs as tests/test_ddc_gpu.py draws them: each even, none a multiple of the hop, a third of
    them shorter than a hop."""
    rng = np.random.default_rng(20_241)
    lens, left = [], narrow
    while left > 0:
        m = 2 * int(rng.integers(1, hop // 2) if rng.random() < 0.35 else rng.integers(hop, 100 * hop))
        m += 2 * (m % hop == 0)
        lens.append(min(m, left))
        left -= lens[-1]
    return lens


def chain(capi, table, corrected, lens=None):
    """The impaired cu8 fixture -> (sums, sdr_iq_correction_from_sums) -> a fresh DDC with that correction (D = 8, T = 64,
    three bands) -> bank (N = 512, hop 128), both on one HIP stream, against the oracle receiver fed the reference's streams
    of the corrected values.  Returns the text of every listener."""
    import torch

    e = Q.E2E
    n, hop, rate, d, frames = e["n"], e["hop"], e["rate"], e["decimation"], e["frames"]
    fix = Q.e2e_reference(table, corrected)
    raw, narrow, ref, outs, decs = fix["raw"], fix["narrow"], fix["ref"], fix["outs"], fix["decs"]
    taps = R.e2e_taps()
    per = 512
    if lens is None:
        lens = [min(per * hop, narrow - a) for a in range(0, narrow, per * hop)]
    assert sum(lens) == narrow and max(lens) <= per * hop
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        wide = torch.from_numpy(raw).cuda()
        out = torch.full((3, narrow, 2), float("nan"), dtype=torch.float32, device="cuda")
        scratch = torch.empty((3, per * hop, 2), dtype=torch.float32, device="cuda")
    stream.synchronize()
    corr = None
    if corrected:
        # the estimate, as a receiver forms it: a DDC with the sums on over the stream, read, from_sums
        probe = capi.Ddc(d, taps, e["steps"], in_format=capi.DDC_CU8, max_in_samples=per * hop * d)
        probe.set_stream(stream.cuda_stream)
        probe.enable_iq_sums(True)
        have = 0
        for m in lens:
            probe.process_device(wide.data_ptr() + have * d * 2, m * d, scratch.data_ptr(), per * hop)
            have += m
        s = probe.read_iq_sums()
        probe.close()
        assert s == Q.sums(raw, R.CU8)
        corr = capi.iq_correction_from_sums(s, capi.DDC_CU8)
        assert bits_equal(np.array(corr.astuple(), np.float32), np.array(fix["corr"], np.float32))
    bank = capi.Bank(rate, n, n_bands=3, edge_width=e["edge"], max_batch_frames=per, max_listeners=2, hop=hop)
    ddc = capi.Ddc(d, taps, e["steps"], in_format=capi.DDC_CU8, max_in_samples=per * hop * d)
    bank.set_stream(stream.cuda_stream)
    ddc.set_stream(stream.cuda_stream)
    ddc.set_iq_correction(corr)
    for b, cf in enumerate(Q.e2e_centers()):
        bank.set_center_frequency(b, cf)
        for lid, bin_ in enumerate(Q.LISTEN[b]):
            assert bank.attach(b, bin_) == lid
    bank.enable_results(True)
    have = done = 0
    batches = []
    for m in lens:
        ddc.process_device(wide.data_ptr() + have * d * 2, m * d, out.data_ptr() + have * 8, narrow)
        have += m
        k = (have - n) // hop + 1 - done if have >= n else 0
        if k == 0:
            continue
        bank.process_device_stream(out.data_ptr() + done * hop * 8, k, narrow)
        batches.append((done, done + k))
        done += k
    ddc.sync()
    bank.sync()
    assert have == narrow and done == frames and len(batches) >= 3 and bank.total_frames == frames
    assert bits_equal(out.cpu().numpy(), ref)
    live = [list(range(len(b))) for b in Q.LISTEN]
    text = [[""] * len(b) for b in Q.LISTEN]
    n_peaks = 0
    for a, z in batches:
        res = bank.poll(wait=True)
        n_peaks += check_batch_polled(res, outs, a, z, 2, text, 3, live=live)[1]
    assert bank.poll() is None and n_peaks > 0
    for b in range(3):
        for lid in live[b]:
            assert text[b][lid] == decs[b][lid][0], (b, lid)
    ddc.close()
    bank.close()
    return text


def check_chain_text(text, ghosts):
    e = Q.E2E
    assert e["calls"][0] in text[0][0] and e["calls"][1] in text[1][0], text
    assert (e["calls"][0] in text[1][1]) == ghosts, text[1][1]


def test_chain_corrected_cut_into_whole_hops(capi, table):
    check_chain_text(chain(capi, table, True), ghosts=False)
    outs = Q.e2e_reference(table, True)["outs"]
    assert all(Q.peaks_near(outs[b], g, 2) == 0 for b in range(3) for g in Q.GHOST_BINS)  # (what the bank delivered: no ghost, no DC line)


def test_chain_corrected_cut_raggedly(capi, table):
    lens = ragged_lengths(Q.e2e_reference(table, True)["narrow"], Q.E2E["hop"])
    assert len(lens) >= 8 and any(m < Q.E2E["hop"] for m in lens)
    check_chain_text(chain(capi, table, True, lens), ghosts=False)


def test_chain_uncorrected_shows_the_ghosts(capi, table):
    check_chain_text(chain(capi, table, False), ghosts=True)
    outs = Q.e2e_reference(table, False)["outs"]
    assert all(Q.peaks_near(outs[b], g, 1) >= 1 for b, g in enumerate(Q.GHOST_BINS))
