"""The controls of a running bank, turned between the batches of a stream, against the oracle bit for bit: signal debounce
(k_set_debounce and the debouncer state k_listen_decode carries under a changing threshold), edge width (the noise geometry
of the scan, of the chains and of the literal path; the read of the batch before a change), peak threshold and peak search,
per band, through the input paths, under a captured graph, with a listen half pending, over a group.  The cases are
tests/setters_gen.py's; tests/test_setters_reach.py shows on the CPU what they reach."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import reports_ref  # noqa: E402
import setters_gen as gen  # noqa: E402
from parity_tools import GROUP_BANDS, Pair, bits_equal, capi, environment  # noqa: E402, F401
from parity_tools import REC_FIELDS  # noqa: E402


def test_debounce_sequence(capi):
    """1 -> 3 -> 1 -> 5 -> 70 -> 2 -> 0 -> 3 on 70 listeners (two workgroups of k_set_debounce) with glitching raw states,
    a single-frame batch, a listener detached in front of a setter, one attached behind one into a slot of its own and one
    into the detached one's slot: debounced bits, edges, text and decoder state are the oracle's."""
    case = gen.case_debounce()
    bank = case.run(capi, min_edges=5)
    assert bank.cfg.max_listeners > 64 and bank.listener_count(0) == gen.DEB_LISTENERS + 1
    bank.close()


def test_debounce_sequence_traced(capi):
    """The same thresholds on listeners that stay (the tap compares raw and debounced bits frame by frame)."""
    bands = [gen.deb_band()]
    steps = [s for s in gen.deb_steps() if s[0] in ("batch", "set")]
    case = gen._case(gen.N, bands, [gen.deb_bins()], steps, gen.DEB_SEED, debounce=1, path="device", trace=True)
    case.run(capi, min_edges=5).close()


def test_per_band(capi):
    """Three bands: debounce and peak threshold of band 1, then of band 2, band 0 untouched; bands -1 and 3 are refused
    (SDR_ERR_BAD_ARG) and change nothing."""
    gen.case_bands().run(capi, min_edges=5).close()


@pytest.mark.parametrize("env", [{}, {"SDR_NOISE_PATH": "chains"}, {"SDR_NOISE_FORCE_EXACT": "1"}], ids=["scan", "chains", "literal"])
def test_edge_width_sequence(capi, env):
    """default -> 1 -> nine windows -> one-bin windows -> 0 -> default, a setter in mid-cumulation and a batch of two
    cumulations, on the noise scan, the chains and the scan's literal path.  Behind every setter the batch before reads back
    with the width it ran with (SDR_OK, the oracle's records, variance included); refused widths change nothing."""
    with environment(**env):
        gen.case_edge().run(capi, min_edges=5).close()


def test_peak_threshold_sequence(capi):
    """Two bands from 15 and 12 dB through 9, 21.5, 0, -3 and +Inf, every change in mid-cumulation, the peak search off for one
    cumulation and on again: peak lists with their frequencies, peak_thr records and deliveries are the oracle's."""
    case = gen.case_peaks()
    bank = case.run(capi, min_edges=5)
    assert case.peaks >= 40
    bank.close()


@pytest.mark.parametrize("row", [r[0] for r in gen.PATH_ROWS])
def test_paths(capi, row):
    """Both sequences, shortened, through staged input, sc16, 8-bit, an overlapped device stream and a windowed bank: the
    setters' order against staged input and the stream carry."""
    gen.case_path(row).run(capi, min_edges=5).close()


def test_graph(capi):
    """Setters between replays: debounce and peak threshold take effect at the next replay with the capture in place; a
    changed edge width makes sdr_graph_launch refuse (SDR_ERR_STATE) until release and capture, after which it holds;
    setting the width the capture has does not invalidate it."""
    case = gen.case_graph()
    bank = case.run(capi, min_edges=5)
    assert bank.graph_batches == gen.GRAPH_BATCHES
    bank.close()


def test_deferred(capi):
    """With a listen half pending sdr_set_signal_debounce is refused (SDR_ERR_STATE) and changes nothing; the peak threshold
    and the edge width are accepted and reach the next batch only.  The pending half, its reports and the batch behind it
    are the oracle's."""
    case = gen.case_deferred()
    case.run_oracle()
    ends = [e for _, e in case.spans]
    wpm = {lid: reports_ref.wpm_at(case.outs[0]["deb"][:, lid], case.rate, case.step, ends, start=case.life[0][lid][0])
           for lid in range(len(case.bins[0]))}
    seen = []

    def reports(bank, k):
        got = bank.poll_reports(wait=True)
        a, e = case.spans[k]
        want = [reports_ref.expected(case.outs[0], 0, lid, case.bins[0][lid], a, e, case.life[0][lid][0], wpm[lid][k]) for lid in case.live(0, a, e)]
        assert got is not None and got[0] == k and len(got[1]) == len(want), f"batch {k}: reports"
        for r, w in zip(got[1], want):
            bad = reports_ref.same(reports_ref.as_dict(r), w)
            assert not bad, f"batch {k} listener {w['listener']}: report fields {bad} differ"
        seen.append(k)

    bank = case.run(capi, min_edges=5, prepare=lambda bank: bank.enable_reports(True), before_poll=reports)
    assert seen == [0, 1, 2]
    bank.close()


def test_group(capi):
    """sdr_group_set_signal_debounce (every band, one band), sdr_group_set_edge_width and sdr_group_set_find_peaks between
    the batches of a group of two members beside one bank of the same five bands: every merged delivery equals the bank's,
    and both equal the oracle's on every band; a band out of range is refused."""
    n, nine = gen.N, gen.nine_window_edge(gen.N)
    batches = (170, 130, 1, 150, 149)
    plan = [[("signal_debounce", -1, 3)], [("signal_debounce", 3, 5), ("edge_width", None, nine)], [("find_peaks", None, False)],
            [("find_peaks", None, True), ("edge_width", None, 1), ("signal_debounce", -1, 0)]]
    bands = [gen.band_input(n, sum(batches), gen.PATH_KINDS, 8800 + b) for b in range(GROUP_BANDS)]
    steps = []
    for frames, calls in zip(batches, plan + [[]]):
        steps.append(("batch", frames))
        for name, band, value in calls:
            steps += [("set", name, b, value) for b in (range(GROUP_BANDS) if band == -1 else [band])]
    case = gen._case(n, bands, [b[2] for b in bands], steps, 8800, debounce=1)
    case.run_oracle()
    case.begin()
    p = Pair(capi, (0, 0), gen.RATE, n, edge_width=gen.EDGE, max_listeners=8, max_batch_frames=max(batches), max_peaks=1024, signal_debounce=1)
    p.bank.enable_results(True)
    p.group.enable_results(True)
    for b in range(GROUP_BANDS):
        p.bank.set_center_frequency(b, case.centers[b])
        m, lb = p.group.member(b)
        m.set_center_frequency(lb, case.centers[b])
        for t in bands[b][2]:
            p.attach(b, t)
    iq = np.stack([b[0] for b in bands])
    pos = 0
    for k, (frames, calls) in enumerate(zip(batches, plan + [[]])):
        p.process(iq[:, pos:pos + frames])
        res = p.polls()
        assert res["batch_index"] == k
        case.check_polled(res, pos, pos + frames)
        for name, band, value in calls:
            if name == "signal_debounce":
                for b in range(GROUP_BANDS) if band == -1 else [band]:
                    p.bank.set_signal_debounce(b, value)
                p.group.set_signal_debounce(band, value)
            else:
                getattr(p.bank, "set_" + name)(value)
                getattr(p.group, "set_" + name)(value)
            if name == "edge_width":  # the batch before, read behind the setter: the width it ran with
                for b in (0, 3):
                    m, lb = p.group.member(b)
                    for got in (m.read_frame_records(lb), p.bank.read_frame_records(b)):
                        for f in REC_FIELDS:
                            assert bits_equal(got[f], case.outs[b]["frames"][f][pos:pos + frames].copy()), f"band {b} batch {k} field {f}"
        p.check_device()
        pos += frames
    for call, args in ((p.group.set_signal_debounce, (GROUP_BANDS, 2)), (p.group.set_signal_debounce, (-2, 2)), (p.group.set_peak_threshold, (GROUP_BANDS, 2.0))):
        with pytest.raises(capi.SdrError) as err:
            call(*args)
        assert err.value.code == capi.ERR_BAD_ARG
    assert p.polls(wait=False) is None
    case.check_end(p.bank, 5)
    for b in range(GROUP_BANDS):
        m, lb = p.group.member(b)
        for lid in range(len(case.bins[b])):
            assert np.array_equal(m.read_decoder_state(lb, lid), case.refs[b].decoder_state(lid)), f"band {b} listener {lid}: the member's decoder"
    p.close()


def test_group_refuses_debounce_with_a_listen_half_pending(capi):
    """sdr_group_set_signal_debounce with a batch waiting for its listen half: SDR_ERR_STATE before any member changes."""
    n = gen.N
    band = gen.band_input(n, 120, gen.PATH_KINDS, 8900)
    group = capi.Group((0, 0), gen.RATE, n, 2, edge_width=gen.EDGE, max_listeners=4, max_batch_frames=120, signal_debounce=1)
    import torch

    group.enable_results(True)
    group.defer_listen(True)
    ts = [torch.from_numpy(band[0][None]).to("cuda:0") for _ in range(2)]
    group.process_device([t.data_ptr() for t in ts], 120)
    for b in (-1, 0, 1):
        with pytest.raises(capi.SdrError) as err:
            group.set_signal_debounce(b, 3)
        assert err.value.code == capi.ERR_STATE
    group.poll_peaks(wait=True)
    group.process_listen()
    group.set_signal_debounce(-1, 3)
    group.sync()
    group.close()
