"""Waterfall rows (sdr_enable_rows / sdr_poll_rows, csrc/k_peaks.hip k_cum_rows): one row per completed cumulation, the
group maxima of the exact cumulation, travelling with its batch.

The expected row is the rule of include/sdrainer_hip.h applied with numpy - the literal loop `m = cum[j G]; v > m -> m = v`,
vectorised over the columns - to the oracle's "cumulation" output (oracle.Receiver.process) and, wherever the batch is still
the bank's last one, to bank.read_cumulation as well.  Both comparisons are bit for bit (uint32 views), NaN positions equal.

Shapes: the geometries the feature's issue names, plus what they do not reach of the kernel: groups of exactly one wave (G =
64), groups that meet in LDS (G = 128) and groups wider than a workgroup (G = 512, two blocks of bins per workgroup).  The
issue's batches of 250, 130 and 170 frames complete 2, 1 and 2 cumulations whatever their order; the batch that completes
none is a fourth one of 30 frames, and a fifth of 40 closes the cumulation it leaves open."""
import functools

import numpy as np
import pytest

import value_range_gen as gen
from parity_case import Case
from parity_tools import (RATES, GROUP_BANDS, Pair, capi, environment, group_bands, listener_bins, make_stream,  # noqa: F401 (capi: the fixture)
                          nan_equal_bits, random_window, same_delivery)

pytestmark = pytest.mark.gpu

STEPS = (250, 130, 170, 30, 40)  # cumulations completed: 2, 1, 2, 0, 1; the second to fifth batch start on a carry


def reduce_row(cum, columns):
    """The rule, literally: per group of G = N / columns adjacent bins, m = first; every later v with v > m replaces it."""
    g = np.asarray(cum, np.float32).reshape(columns, -1)
    m = g[:, 0].copy()
    with np.errstate(invalid="ignore"):
        for k in range(1, g.shape[1]):
            v = g[:, k]
            sel = v > m
            m[sel] = v[sel]
    return m


def test_the_rule_on_the_host():
    """(no GPU work) NaN first, NaN further in, all -inf, +inf, and a group of one."""
    nan, inf = np.float32("nan"), np.float32("inf")
    cum = np.array([nan, 5, 7, 1, 2, nan, 9, 3, -inf, -inf, -inf, -inf, 1, inf, nan, 2], np.float32)
    got = reduce_row(cum, 4)
    assert np.isnan(got[0]) and got[1] == 9 and got[2] == -inf and got[3] == inf
    assert nan_equal_bits(reduce_row(cum, 16), cum)


def streams_case(n, n_bands, steps, tones, listeners, sc16, seed, path=None, hop=None, windows=None, bands=None):
    """A Case over keyed carriers (parity_tools.make_stream: float32 and, for sc16, the int16 behind it), without trace."""
    made = bands or [make_stream(n, hop or n, sum(steps), RATES[n], tones, seed + 17 * b, sc16) for b in range(n_bands)]
    return Case(n, n_bands, None, 0, [("batch", x) for x in steps], seed, rate=RATES[n], max_listeners=listeners,
                path=path or ("device_sc16" if sc16 else "device"), bands=made, init_bins=[listener_bins(n, m[2], listeners) for m in made],
                hop=hop, windows=windows)


@functools.lru_cache(maxsize=None)
def small_case(n, sc16):
    """Two bands, 8 tones, the five batches; the oracle's run is shared by every test that uses the geometry."""
    case = streams_case(n, 2, STEPS, 8, 8, sc16, seed=4100 + n)
    case.run_oracle()
    return case


def chunk_keys(res):
    return [(int(ch["band"]), int(ch["frame"])) for ch in res["chunks"]]


def expected_row(case, band, frame, columns):
    out = case.outs[band]
    return reduce_row(out["cumulation"][list(out["peak_frames"]).index(frame)], columns)


def check_rows(case, bank, rows, res, columns, read_back):
    """The rows of one batch against the oracle, in the order of the batch's chunks; read_back: the batch is the bank's last,
    and the same rule over sdr_read_cumulation must match too."""
    keys = chunk_keys(res)
    assert rows.shape == (len(keys), columns), f"batch {res['batch_index']}: {rows.shape} rows for {len(keys)} chunks"
    local = {}
    for row, (band, frame) in zip(rows, keys):
        c = local[band] = local.get(band, -1) + 1
        if case is not None and hasattr(case, "outs"):
            want = expected_row(case, band, frame, columns)
            assert nan_equal_bits(row, want), \
                f"band {band} cumulation at frame {frame}: columns {np.flatnonzero(row.view(np.uint32) != want.view(np.uint32))[:8]} differ from the oracle's"
        if read_back:
            assert nan_equal_bits(row, reduce_row(bank.read_cumulation(band, c), columns)), f"band {band} chunk {c}: differs from sdr_read_cumulation"
    return {k: r for k, r in zip(keys, rows)}


def run_rows(capi, case, columns, read_back=True, check_polled=True, env=None):
    """Every batch of the case on a new bank with rows on: poll_rows first (a peek), then poll, which must hand out the same
    batch with its chunks as ever.  Returns the bank and {(band, completing frame): row}."""
    with environment(**(env or {})):
        bank = case.new_bank(capi)
    bank.enable_rows(columns)
    assert bank.row_columns == columns
    got = {}
    for k, (a, e) in enumerate(case.spans):
        case.set_window(bank, k)
        keep = case._enqueue(bank, a, e)
        peek = bank.poll_rows(wait=True)
        assert peek is not None and peek[0] == k, f"batch {k}: poll_rows looked at {peek and peek[0]}"
        again = bank.poll_rows(wait=False)
        assert again[0] == k and again[1].tobytes() == peek[1].tobytes(), f"batch {k}: a second peek differs"
        res = bank.poll(wait=True)
        assert res["batch_index"] == k, f"batch {k}: poll delivered {res['batch_index']} after the peek"
        if check_polled and hasattr(case, "outs"):
            case.check_polled(res, a, e)
        want_chunks = (a % 100 + (e - a)) // 100 * case.n_bands
        assert len(res["chunks"]) == want_chunks, f"batch {k}: {len(res['chunks'])} chunks"
        got.update(check_rows(case, bank, peek[1], res, columns, read_back))
        del keep
    assert bank.poll_rows(wait=False) is None and bank.poll(wait=False) is None
    return bank, got


@pytest.mark.parametrize("sc16", [False, True], ids=["f32", "sc16"])
@pytest.mark.parametrize("n, columns", [(512, 64), (512, 512), (4096, 256)])
def test_small_geometries(capi, n, columns, sc16):
    case = small_case(n, sc16)
    bank, got = run_rows(capi, case, columns)
    assert len(got) == 2 * 6 and sum(len(p) for o in case.outs for p in o["peaks"]) > 0
    bank.close()


@pytest.mark.parametrize("n, columns, env", [
    (4096, 64, {}),                        # G = 64: the whole wave is one group
    (8192, 64, {}),                        # G = 128: two waves meet in LDS, two columns per workgroup
    (32768, 64, {}),                       # G = 512: a workgroup walks two blocks of bins
    (16384, 1024, {"SDR_FFT_R32": "1"}),   # through k_fft_r32
    (65536, 2048, {}),
], ids=lambda v: str(v) if isinstance(v, int) else "")
def test_group_widths_and_large_geometries(capi, n, columns, env):
    steps = {16384: (230,), 65536: (210,)}.get(n, (130, 90))  # (one batch of two cumulations; else a carry into the second batch)
    case = streams_case(n, 1, steps, 8, 8, False, seed=4200 + n)
    case.run_oracle()
    bank, got = run_rows(capi, case, columns, env=env)
    assert len(got) == sum(steps) // 100
    bank.close()


def test_overlap_and_window(capi):
    """N = 4096, hop 1024, a window: the rows follow the windowed, overlapped frames (sdr_process_device_stream)."""
    n, hop, steps = 4096, 1024, (230, 130)
    w = random_window(n, 77)
    case = streams_case(n, 1, steps, 8, 8, False, seed=4300, hop=hop, windows=[w, w])
    case.run_oracle()
    bank, got = run_rows(capi, case, 256, check_polled=False)  # (text and rune frames of a hop are parity_case's timed checks)
    assert len(got) == 3
    bank.close()


def test_split_invariance(capi):
    """The same stream in other batches: the same rows for the same cumulations."""
    case = small_case(512, False)
    _, first = run_rows(capi, case, 64, read_back=False)
    other = streams_case(512, 2, (100, 320, 1, 199), 8, 8, False, seed=0, bands=[(case.stream[b], None, case.carriers[b]) for b in range(2)])
    other.outs = case.outs  # (the same input: the same oracle stream; nothing of `other` but its batches differs)
    bank, second = run_rows(capi, other, 64, read_back=False, check_polled=False)
    assert first.keys() == second.keys() and all(first[k].tobytes() == second[k].tobytes() for k in first)
    bank.close()


def test_non_finite_groups(capi):
    """Groups whose first bin cumulates to NaN, with a NaN further in, all -inf, and with +inf - through the public input:
    frames 0 - 49 are placed where psd words round to zero (tests/value_range_gen.py "floor": dB of -inf), the rest where
    the keyed carriers overflow ("carrier_inf": +inf).  A carrier's bin then sums -inf and +inf in the first cumulation
    (NaN; bin 256 opens its group of 8, bins 78 and 434 sit inside theirs), a noise bin -inf; the second cumulation holds
    +inf at the carriers and finite values elsewhere.  The oracle's cumulation decides, and is checked first."""
    n, frames, seed, columns = 512, 200, 9008, 64
    iq, bins = gen.base(n, frames, seed)
    k = np.where(np.arange(frames) < 50, gen.exponents("floor", n, frames, seed), gen.exponents("carrier_inf", n, frames, seed))
    case = Case(n, 1, None, 0, [("batch", 130), ("batch", 70)], seed, rate=gen.RATES[n], bands=[(gen.scale(iq, k), None, bins)],
                init_bins=[gen.listeners(n, bins)], nan_ok=True)
    case.run_oracle()
    g = np.stack(case.outs[0]["cumulation"]).reshape(2, columns, -1)
    nan = np.isnan(g)
    assert nan[0, :, 0].any(), "no group opens with NaN"
    assert (~nan[0, :, 0] & nan[0].any(1)).any(), "no group holds a NaN behind its first bin"
    assert (g[0] == -np.inf).all(1).any(), "no group is all -inf"
    assert ((g[1] == np.inf).any(1) & ~nan[1].any(1)).any(), "no group holds +inf"
    for cols in (columns, n):  # (G = 8, and G = 1: every NaN bin is its group's first)
        bank, got = run_rows(capi, case, cols, check_polled=False)
        assert len(got) == 2
        bank.close()


def test_delivery(capi):
    case = small_case(512, False)
    # enable_rows needs results, and a valid column count
    bare = capi.Bank(case.rate, 512, n_bands=2, max_batch_frames=256)
    with pytest.raises(capi.SdrError) as e:
        bare.enable_rows(64)
    assert e.value.code == capi.ERR_STATE
    bare.enable_results(True)
    for bad in (3, 32, 2 * 512, -64, 96):
        with pytest.raises(capi.SdrError) as e:
            bare.enable_rows(bad)
        assert e.value.code == capi.ERR_BAD_ARG, bad
    assert bare.row_columns == 0
    bare.close()

    bank = case.new_bank(capi)
    bank.enable_rows(64)
    # a buffer too small: ERR_BAD_SIZE with the rows needed, nothing delivered; the next call delivers
    keep = case._enqueue(bank, *case.spans[0])
    for cap in (0, 3):
        with pytest.raises(capi.SdrError) as e:
            bank.poll_rows(wait=True, rows_cap=cap)
        assert e.value.code == capi.ERR_BAD_SIZE and e.value.n_rows == 4
    k, rows = bank.poll_rows(wait=True, rows_cap=4)
    res = bank.poll(wait=True)
    assert k == 0 and res["batch_index"] == 0
    case.check_polled(res, *case.spans[0])
    check_rows(case, bank, rows, res, 64, True)
    # a batch processed with rows off has none, and the setting comes back with the next batch
    bank.enable_rows(0)
    keep = case._enqueue(bank, *case.spans[1])
    bank.enable_rows(64)
    k, rows = bank.poll_rows(wait=True)
    assert k == 1 and rows.shape == (0, 64)
    case.check_polled(bank.poll(wait=True), *case.spans[1])
    keep = case._enqueue(bank, *case.spans[2])
    k, rows = bank.poll_rows(wait=True)
    res = bank.poll(wait=True)
    case.check_polled(res, *case.spans[2])
    assert k == 2 and len(check_rows(case, bank, rows, res, 64, True)) == 4
    del keep
    bank.close()


def test_parked_batches_keep_their_rows(capi):
    """Eight batches without a poll on a ring of six sets: the first two are parked when their sets are reused, and every
    batch's rows still arrive, oldest first, each in front of its batch."""
    steps = (130,) * 8
    case = streams_case(512, 2, steps, 8, 8, False, seed=4400)
    case.run_oracle()
    bank = case.new_bank(capi)
    bank.enable_rows(64)
    keep = [case._enqueue(bank, a, e) for a, e in case.spans]
    assert bank.results_pending == 8
    n_rows = 0
    for k, (a, e) in enumerate(case.spans):
        peek = bank.poll_rows(wait=True)
        res = bank.poll(wait=True)
        assert peek[0] == k and res["batch_index"] == k
        case.check_polled(res, a, e)
        n_rows += len(check_rows(case, bank, peek[1], res, 64, k == len(steps) - 1))
    assert n_rows == 2 * (sum(steps) // 100) and bank.poll_rows(wait=False) is None
    del keep
    bank.close()


def test_deferred_listen(capi):
    """The rows belong to the spectral half: readable between sdr_poll_peaks and sdr_process_listen."""
    case = small_case(512, False)
    bank = case.new_bank(capi)
    bank.enable_rows(64)
    bank.defer_listen(True)
    a, e = case.spans[0]
    keep = case._enqueue(bank, a, e)
    with pytest.raises(capi.SdrError) as err:
        bank.enable_rows(128)
    assert err.value.code == capi.ERR_STATE  # a listen half is pending
    pk = bank.poll_peaks(wait=True)
    k, rows = bank.poll_rows(wait=True)
    assert k == 0 and pk["batch_index"] == 0 and bank.poll(wait=False) is None
    check_rows(case, bank, rows, pk, 64, False)
    bank.process_listen()
    k2, rows2 = bank.poll_rows(wait=True)
    res = bank.poll(wait=True)
    assert k2 == 0 and rows2.tobytes() == rows.tobytes() and res["batch_index"] == 0
    case.check_polled(res, a, e)
    del keep
    bank.close()


def test_graph(capi):
    """Two replays of six batches of 120 frames at N = 4096 (cumulations straddle batches and replays) against an eager bank
    fed the same input - and against the oracle; enable_rows after a capture invalidates it."""
    import torch

    n, per, columns = 4096, 120, 256
    made = [make_stream(n, n, 12 * per, RATES[n], 8, 4500, False)]
    eager = streams_case(n, 1, (per,) * 12, 8, 8, False, seed=4500, bands=made)
    eager.run_oracle()
    bank, want = run_rows(capi, eager, columns, read_back=False)
    bank.close()
    case = streams_case(n, 1, (per,) * 12, 8, 8, False, seed=4500, bands=made, path="graph")
    case.outs = eager.outs
    bank = case.new_bank(capi, torch.cuda.Stream())
    bank.enable_rows(columns)
    bank.graph_capture(per)
    got, k = {}, 0
    for replay in range(2):
        spans = case.spans[6 * replay:6 * replay + 6]
        batches = [case.device_batch(a, e) for a, e in spans]
        torch.cuda.synchronize()
        bank.graph_launch([x.data_ptr() for x in batches])
        for a, e in spans:
            peek = bank.poll_rows(wait=True)
            res = bank.poll(wait=True)
            assert peek[0] == k and res["batch_index"] == k
            case.check_polled(res, a, e)
            got.update(check_rows(case, bank, peek[1], res, columns, False))
            k += 1
        bank.sync()
    assert got.keys() == want.keys() and len(got) == 14 and all(got[key].tobytes() == want[key].tobytes() for key in got)
    bank.enable_rows(0)
    with pytest.raises(capi.SdrError) as e:
        bank.graph_launch([x.data_ptr() for x in batches])
    assert e.value.code == capi.ERR_STATE
    bank.close()


def test_group(capi):
    """Two members on one GPU, five bands: the merged rows equal one bank's for the same bands, in `chunks` order."""
    n, rate, columns = 512, RATES[512], 64
    iq, bins = group_bands(380, rate, n, 4, seed=4600)
    pair = Pair(capi, [0, 0], rate, n, max_batch_frames=256, max_listeners=4)
    for b in range(GROUP_BANDS):
        for bn in bins[b]:
            pair.attach(b, bn)
    pair.bank.enable_results(True)
    pair.group.enable_results(True)
    with pytest.raises(capi.SdrError) as e:
        pair.group.enable_rows(48)
    assert e.value.code == capi.ERR_BAD_ARG
    pair.bank.enable_rows(columns)
    pair.group.enable_rows(columns)
    for k, (a, e) in enumerate([(0, 250), (250, 380)]):
        pair.process(iq[:, a:e])
        one, merged = pair.bank.poll_rows(wait=True), pair.group.poll_rows(wait=True)
        assert one[0] == merged[0] == k and one[1].shape == merged[1].shape == (GROUP_BANDS * (2, 1)[k], columns)
        assert one[1].tobytes() == merged[1].tobytes(), f"batch {k}: the group's rows differ from the bank's"
        res = pair.polls()
        assert res["batch_index"] == k and [int(c["band"]) for c in res["chunks"]] == sorted(int(c["band"]) for c in res["chunks"])
    assert pair.group.poll_rows(wait=False) is None
    pair.close()


def test_unchanged_path(capi):
    """Rows off: no launch of the new stage in the profile, and the results of a bank that had rows on and off again are
    byte for byte those of a bank that never heard of rows.  Rows on: one launch per batch that completes a cumulation."""
    case = small_case(512, False)
    banks = [case.new_bank(capi) for _ in range(3)]
    banks[1].enable_rows(64)
    banks[1].enable_rows(0)
    banks[2].enable_rows(64)
    assert capi.load().sdr_kernel_name(8) == b"k_cum_rows" and [capi.load().sdr_kernel_name(i).decode() for i in range(8)] == list(capi.KERNELS)
    for b in banks:
        b.profile_enable(True)
    for a, e in case.spans:
        keep = [case._enqueue(b, a, e) for b in banks]
        plain, off, on = [b.poll(wait=True) for b in banks]
        same_delivery(off, plain)
        same_delivery(on, plain)
        del keep
    prof = [b.profile_read() for b in banks]
    assert prof[0]["k_cum_rows"] == (0.0, 0) and prof[1]["k_cum_rows"] == (0.0, 0)
    assert prof[2]["k_cum_rows"][1] == 4 and prof[2]["k_cum_rows"][0] > 0
    for name in capi.KERNELS:
        assert prof[0][name][1] == prof[1][name][1] == prof[2][name][1], name
    for b in banks:
        b.close()
