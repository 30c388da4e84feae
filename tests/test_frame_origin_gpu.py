"""The 32-bit frame words of the kernels across 2^31 and 2^32: banks that start at 2^31 - 48, 2^32 - 96 and 5 * 2^32 - 80
(sdr_set_first_frame), every case against the CPU oracle through parity_case.Case with first_frame set - the oracle counts
from 0 and every expected frame is shifted: first_frame, chunk frames, scope frames and total_frames as int64, edge and rune
frames modulo 2^32, sdr_attach_at start frames given shifted.  What is no frame number is what it is from frame 0.

The cases and their inputs are tests/frame_origin_gen.py's; tests/test_frame_origin_reach.py asserts on the CPU that each
has a listener with an edge and a rune on both sides of its crossing.  What they pin: `skip` and `untapped` of
k_listen_gather, k_listen_decode and k_report_marks as signed differences on both sides of the wrap; the marks
k_listen_decode moves along behind every batch; the casts of sdr_attach, sdr_attach_at (and its int64 range check),
k_listener_stop's stamp, the graph cursors, the chunk frames of capi_results.hip, the scope reads and the group's agreement
on first_frame.  Every comparison is exact."""
import numpy as np
import pytest

import frame_origin_gen as fo
import reports_ref as ref
from parity_tools import capi, frames32, same_delivery, transitions  # noqa: F401 (capi: the fixture)

pytestmark = pytest.mark.gpu


def run(capi, case, **kw):
    bank = case.run(capi, min_edges=5, **kw)
    assert bank.total_frames == case.first_frame + case.total
    return bank


@pytest.mark.parametrize("debounce", [1, 5])
@pytest.mark.parametrize("where", ["on", "in"])
@pytest.mark.parametrize("origin", fo.ORIGINS)
def test_eager_batches(capi, origin, where, debounce):
    """The crossing on a batch boundary with a one-frame batch behind it, and inside a batch at no word end; keyed carriers
    and an idle listener carried across; edges, runes and their frames, trace, decoder state, chunk frames."""
    run(capi, fo.eager(origin, where, debounce)).close()


@pytest.mark.parametrize("origin", [fo.O31, fo.O32])
def test_attach_and_detach_around_the_crossing(capi, origin):
    """sdr_attach on the batch boundary in front of the crossing (a new slot) and on the one at it (the slot of a listener
    detached before it: a brand-new decoder whose start frame is the multiple of 2^31), and one frame on."""
    case = fo.attach_detach(origin)
    bank = run(capi, case)
    # the heir's runes belong to its own decoder: a new one over its bits from the crossing on
    from parity_tools import decode
    c = fo.crossing(origin)
    text, _, at = decode(case.outs[0]["deb"][c:, 5], case.rate, case.step)
    assert case.text[0][5] == text and len(text) > 3
    assert np.array_equal(np.array(case.rune_at[0][5], np.int64), frames32(at + c, origin))
    bank.close()


def test_stop_behind_the_crossing(capi):
    """sdr_listener_stop between two batches behind the crossing: the character it flushes is stamped with the last frame
    processed, shifted (Case checks every rune frame against the stopped decoder)."""
    case = fo.stop(fo.O32)
    bank = run(capi, case)
    cut = fo.stop_cut()
    assert int(frames32([cut - 1], fo.O32)[0]) in case.rune_at[0][0]
    bank.close()


@pytest.mark.parametrize("wide", [False, True], ids=["n512_1band", "n2048_2bands"])
def test_deferred_batch_straddles_the_crossing(capi, wide):
    """sdr_attach_at with start frames before the crossing, at it, behind it and at the next frame, in a waiting batch that
    straddles it: N = 512 on one band (the small plan: the gather on the peaks stream) from 2^31 - 48, N = 2048 on two
    bands from 2^32 - 96."""
    case = fo.deferred(fo.O32 if wide else fo.O31, wide)
    bank = run(capi, case)
    for band in range(case.n_bands):
        assert all(len(case.text[band][lid]) > 0 for lid in range(3, 7)), "a listener bound inside the batch wrote nothing"
    bank.close()


@pytest.mark.parametrize("origin", [fo.O31, fo.O32, fo.O5])
def test_attach_at_outside_the_waiting_batch(capi, origin):
    """One frame in front of the waiting batch and one frame behind the next frame: SDR_ERR_BAD_ARG, as from frame 0; the
    batch's first frame and the next frame are taken."""
    case = fo.deferred(origin)
    bank = case.new_bank(capi)
    (a0, e0), (a, e) = case.spans[:2]
    keep = [case._enqueue(bank, a0, e0)]
    assert bank.poll(wait=True)["first_frame"] == origin
    bank.defer_listen(True)
    keep.append(case._enqueue(bank, a, e))
    assert bank.poll_peaks(wait=True)["first_frame"] == origin + a
    for bad in (origin + a - 1, origin + e + 1, a, e, (origin + a) % 2 ** 32 if origin >= 2 ** 32 else origin + a + 2 ** 32):
        with pytest.raises(capi.SdrError) as err:
            bank.attach_at(0, case.carriers[0][1], bad)
        assert err.value.code == capi.ERR_BAD_ARG, (bad, err.value)
    n = len(case.init_bins[0])
    assert bank.attach_at(0, case.carriers[0][1], origin + a) == n and bank.attach_at(0, case.carriers[0][2], origin + e) == n + 1
    bank.process_listen()
    res = bank.poll(wait=True)
    assert res["first_frame"] == origin + a and res["n_frames"] == e - a
    bank.close()


@pytest.mark.parametrize("sc16", [False, True], ids=["f32", "sc16"])
def test_graph_replay(capi, sc16):
    """One replay of six batches whose cursors straddle 2^32."""
    run(capi, fo.graph(fo.O32, sc16)).close()


def test_overlapped_frames(capi):
    """N = 512 at a hop of 128 on the device stream path, 2^32 inside the first call."""
    run(capi, fo.overlapped(fo.O32)).close()


@pytest.mark.parametrize("origin", [fo.O31, fo.O32])
def test_reports_and_rows(capi, origin):
    """Reports and rows on from 2^31 - 48 and from 2^32 - 96 (where k_report_marks' differences wrap as unsigned words too):
    the ticks of the listeners bound inside the straddling batch on either side of the crossing, every record against tests/reports_ref.py, the records of the batches adding up to the stream's; the
    rows' batch_index and the chunk frames, every row the group maxima of the oracle's exact cumulation."""
    columns = 64
    case = fo.reports_rows(origin)
    case.run_oracle()
    out, ends = case.outs[0], [e for _, e in case.spans]
    wpm = [ref.wpm_at(out["deb"][:, lid], case.rate, case.step, ends, start=case.life[0][lid][0]) for lid in range(len(case.bins[0]))]
    bank = case.new_bank(capi)
    bank.enable_rows(columns)
    bank.enable_reports(True)
    totals, keep = {}, []
    batches = [s for s in case.steps if s[0] in ("batch", "defer")]
    for k, ((a, e), s) in enumerate(zip(case.spans, batches)):
        if s[0] == "defer":
            bank.defer_listen(True)
            keep.append(case._enqueue(bank, a, e))
            assert bank.poll_peaks(wait=True)["first_frame"] == origin + a
            for _, bn, at in s[2]:
                bank.attach_at(0, int(bn), origin + at)
            bank.process_listen()
            bank.defer_listen(False)
        else:
            keep.append(case._enqueue(bank, a, e))
        k_rep, recs = bank.poll_reports(wait=True)
        k_rows, rows = bank.poll_rows(wait=True)
        res = bank.poll(wait=True)
        assert k_rep == k_rows == res["batch_index"] == k, (k_rep, k_rows, res["batch_index"], k)
        case.check_polled(res, a, e)  # (first_frame, the chunk frames as int64, edge and rune frames)
        live = case.live(0, a, e)
        assert [int(r["listener"]) for r in recs] == live
        for r, lid in zip(recs, live):
            start = case.life[0][lid][0]
            want = ref.expected(out, 0, lid, case.bins[0][lid], a, e, start, wpm[lid][k])
            assert want["ticks"] == e - max(a, start)
            bad = ref.same(ref.as_dict(r), want)
            assert not bad, f"batch {k} listener {lid}: fields {bad} differ: {ref.as_dict(r)} != {want}"
            totals[lid] = ref.add(totals.get(lid), ref.as_dict(r))
        assert [int(ch["frame"]) for ch in res["chunks"]] == [origin + f for f in out["peak_frames"] if a <= f < e]
        assert rows.shape == (len(res["chunks"]), columns)
        for row, ch in zip(rows, res["chunks"]):
            cum = out["cumulation"][list(out["peak_frames"]).index(int(ch["frame"]) - origin)]
            assert not np.isnan(cum).any()  # (so the rule of the rows is a plain maximum per group)
            assert np.array_equal(row.view(np.uint32), cum.reshape(columns, -1).max(axis=1).view(np.uint32)), f"row of frame {ch['frame']}"
    for lid in range(len(case.bins[0])):
        start = case.life[0][lid][0]
        whole = ref.expected(out, 0, lid, case.bins[0][lid], 0, case.total, start, wpm[lid][-1])
        assert not ref.same(totals[lid], whole), f"listener {lid}: the batches' records do not add up: {totals[lid]} != {whole}"
    case.check_end(bank, 5)
    bank.close()


def test_trace_reads(capi):
    """From 5 * 2^32 - 80, the last batch straddling the crossing: the int64 frames of sdr_scope_read_spectral and
    sdr_scope_read_decode (a listener bound inside the batch ticks from its start frame), and sdr_read_edges."""
    origin = fo.O5
    case = fo.traced(origin)
    bank = run(capi, case)
    a, e = case.spans[-1]
    out = case.outs[0]
    assert bank.last_batch_chunks == 2
    for c, f in enumerate((99, 199)):
        hdr, vals = bank.scope_spectral_frame(0, c)
        assert hdr["frame"] == origin + f and hdr["frame"] >> 32 == 5 and hdr["n_values"] == case.n
        assert np.array_equal(vals, out["cumulation"][list(out["peak_frames"]).index(f)].astype(np.float64) * (1.0 / 100.0))
    for lid in case.live(0, a, e):
        start = max(a, case.life[0][lid][0])
        fr = bank.scope_decode_frames(0, lid)
        assert fr["frame"].dtype == np.int64 and np.array_equal(fr["frame"], origin + np.arange(start, e)), f"listener {lid} decode frames"
        assert np.array_equal(fr["state"], out["deb"][start:e, lid].astype(np.float64)), f"listener {lid} decode states"
        trans, states = transitions(out["deb"][:, lid], a, e)
        ed = bank.read_edges(0, lid)
        assert np.array_equal(ed["frame"].astype(np.int64), frames32(trans, origin)) and np.array_equal(ed["state"], states), f"listener {lid} edges"
    late = len(case.bins[0]) - 1
    assert case.life[0][late][0] == fo.crossing(origin) + 10 and len(bank.scope_decode_frames(0, late)) == e - case.life[0][late][0]
    bank.close()


def group_of(capi, case):
    g = capi.Group([0, 0], case.rate, case.n, case.n_bands, edge_width=case.edge, max_batch_frames=case.max_frames,
                   max_listeners=case.max_listeners, max_peaks=case.max_peaks)
    return g


def member_batches(case, a, e):
    import torch

    n = case.n
    return [torch.from_numpy(np.ascontiguousarray(case.stream[m][a * n:e * n]).reshape(1, e - a, 2 * n)).cuda() for m in range(case.n_bands)]


def test_group(capi):
    """Two members on device 0 from 2^32 - 96 (sdr_group_set_first_frame): the merged poll against the oracle."""
    origin = fo.O32
    case = fo.grouped(origin)
    case.run_oracle()
    g = group_of(capi, case)
    g.set_first_frame(origin)
    for b in range(case.n_bands):
        m, lb = g.member(b)
        assert m.total_frames == origin
        m.set_center_frequency(lb, case.centers[b])
        for i, bn in enumerate(case.init_bins[b]):
            assert m.attach(lb, int(bn)) == i
    with pytest.raises(capi.SdrError) as err:
        g.set_first_frame(0)  # (the members hold listeners)
    assert err.value.code == capi.ERR_STATE
    g.enable_results(True)
    case.begin()
    for k, (a, e) in enumerate(case.spans):
        ts = member_batches(case, a, e)
        g.process_device([t.data_ptr() for t in ts], e - a)
        res = g.poll(wait=True)
        assert res["batch_index"] == k
        case.check_polled(res, a, e)
    for b in range(case.n_bands):
        m, lb = g.member(b)
        assert m.total_frames == origin + case.total
        for lid in range(len(case.bins[b])):
            assert case.text[b][lid] == case.refs[b].text(lid), f"band {b} listener {lid} text"
    assert case.edges > 20 and case.peaks > 0 and g.read_drop_counters() == (0, 0)
    g.close()


def test_group_members_that_disagree(capi):
    """Members given different first frames by hand, through sdr_group_member: sdr_group_poll returns SDR_ERR_STATE."""
    case = fo.grouped(fo.O32)
    g = group_of(capi, case)
    g.member(0)[0].set_first_frame(fo.O32)
    g.member(1)[0].set_first_frame(fo.O31)
    g.enable_results(True)
    a, e = case.spans[0]
    ts = member_batches(case, a, e)
    g.process_device([t.data_ptr() for t in ts], e - a)
    with pytest.raises(capi.SdrError) as err:
        g.poll(wait=True)
    assert err.value.code == capi.ERR_STATE
    g.close()


def refused(capi, bank, frame, code):
    with pytest.raises(capi.SdrError) as err:
        bank.set_first_frame(frame)
    assert err.value.code == code, err.value
    return True


def test_the_setters_contract(capi):
    import torch

    f32, _, bins = fo.band()

    def fresh():
        return capi.Bank(fo.RATE, fo.N, max_batch_frames=64, max_listeners=4)
    bank = fresh()
    assert refused(capi, bank, -100, capi.ERR_BAD_ARG) and refused(capi, bank, 150, capi.ERR_BAD_ARG) and bank.total_frames == 0
    bank.set_first_frame(fo.O5)
    bank.set_first_frame(fo.O32)  # (still fresh: it may be set again)
    assert bank.total_frames == fo.O32
    bank.process_host(f32[:1])
    assert refused(capi, bank, fo.O31, capi.ERR_STATE) and bank.total_frames == fo.O32 + 1  # a processed frame
    bank.close()
    bank = fresh()
    assert bank.push_iq(0, fo.RATE, f32[:1]) == 0
    assert refused(capi, bank, fo.O31, capi.ERR_STATE)  # a staged push
    bank.close()
    bank = fresh()
    bank.attach(0, bins[0])
    assert refused(capi, bank, fo.O31, capi.ERR_STATE)  # an attach
    bank.close()
    bank = fresh()
    bank.set_stream(torch.cuda.Stream().cuda_stream)
    bank.graph_capture(16)
    assert refused(capi, bank, fo.O31, capi.ERR_STATE)  # a captured graph
    bank.graph_release()
    bank.set_first_frame(fo.O31)
    assert bank.total_frames == fo.O31
    bank.close()


def unshifted(res, origin):
    """A delivery with every frame number taken back by `origin`: first_frame and the chunk frames as int64, edge and rune
    frames modulo 2^32."""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in res.items()}
    out["first_frame"] -= origin
    out["chunks"]["frame"] -= origin
    out["edges"]["frame"] = ((out["edges"]["frame"].astype(np.int64) - origin) % 2 ** 32).astype(np.uint32)
    out["rune_frames"] = ((out["rune_frames"].astype(np.int64) - origin) % 2 ** 32).astype(np.uint32)
    return out


@pytest.mark.parametrize("origin", (0,) + fo.ORIGINS)
def test_runs_differ_in_frame_numbers_only(capi, origin):
    """The same stream from frame 0 on a bank nobody told about frames, and from `origin` (0: the call is a no-op): the
    deliveries are equal byte for byte once every frame number is taken back by the origin."""
    case = fo.eager(fo.O31, "in", 1)  # (its stream and listeners; the origin is the parameter's)
    deliveries = []
    for first in (None, origin):
        bank = capi.Bank(case.rate, case.n, edge_width=case.edge, max_batch_frames=case.max_frames, max_listeners=case.max_listeners)
        if first is not None:
            bank.set_first_frame(first)
        for bn in case.init_bins[0]:
            bank.attach(0, int(bn))
        bank.enable_results(True)
        got = []
        for a, e in case.spans:
            bank.process_host(case.stream[0][a * case.n:e * case.n])
            got.append(bank.poll(wait=True))
        assert bank.total_frames == (first or 0) + case.total
        deliveries.append(got)
        bank.close()
    for plain, moved in zip(*deliveries):
        assert moved["first_frame"] == plain["first_frame"] + origin
        same_delivery(unshifted(moved, origin), plain)
    assert sum(len(r["runes"]) for r in deliveries[0]) > 20 and sum(len(r["edges"]) for r in deliveries[0]) > 100
