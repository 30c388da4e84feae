"""What the inputs of tests/test_setters_gpu.py reach, from the CPU oracle alone (tests/setters_gen.py holds the table both
sides read): the debounce sequence tells the reference's SetThreshold - the threshold and nothing else - from two wrong
debouncers, down to the decoded text; the edge-width sequence moves the minimum window and the window count; the peak
thresholds change the peak lists.  A later edit of a seed, a kind or a cut that takes a case off what it is there for fails
here, without a GPU."""
import functools

import numpy as np

import setters_gen as gen
from oracle import oracle as orc


@functools.lru_cache(maxsize=None)
def debounce_case():
    case = gen.case_debounce()
    case.run_oracle()
    return case


def listener_sets(case, lid):
    """(first frame, end, [(frame, threshold)]) of a listener of the debounce case: the setters that reach it are those
    called while it is attached - an attach behind a setter at the same frame comes after it, a detach in front before."""
    start, gone = case.life[0][lid]
    end = case.total if gone is None else gone
    return start, end, [(f, v) for f, name, v, _ in case.outs[0]["sets"] if name == "signal_debounce" and start < f < end]


def text_of(case, bits):
    d = orc.Decoder(case.rate, case.n)
    d.reset()
    d.ticks(bits)
    return d.text()


def test_debounce_sequence_tells_wrong_debouncers_apart():
    """The literal debouncer replays the oracle's debounced bits from its raw ones for every listener.  One that zeroes
    its state at a setter and one that keeps counting through the pass-through each differ from it for some listener, in
    the bits, in the edges and in the decoded text."""
    case = debounce_case()
    raw, deb = case.outs[0]["raw"], case.outs[0]["deb"]
    assert [v for _, _, v, _ in case.outs[0]["sets"]] == list(gen.DEB_VALUES) and case.debounce == 1
    differ = {"zeroing": [0, 0, 0], "counting": [0, 0, 0]}  # listeners whose bits / edge count / text differ
    for lid in range(len(case.bins[0])):
        start, end, sets = listener_sets(case, lid)
        want = deb[start:end, lid]
        assert np.array_equal(gen.replay_debounce(raw[:end, lid], start, 1, sets), want), f"listener {lid}: the literal debouncer"
        for wrong, n in differ.items():
            got = gen.replay_debounce(raw[:end, lid], start, 1, sets, wrong)
            if not np.array_equal(got, want):
                n[0] += 1
                n[1] += np.count_nonzero(np.diff(got.astype(np.int8))) != np.count_nonzero(np.diff(want.astype(np.int8)))
                n[2] += text_of(case, got) != text_of(case, want)
    assert all(min(n) >= 1 for n in differ.values()), differ


def test_debounce_sequence_state_at_the_setters():
    """A raw run is in progress at every setter; the 5 -> 70 setter finds a stateCount of 5 to 69 somewhere; the second
    workgroup of k_set_debounce (slots 64 and up) holds listeners the debouncer changes; the listener attached behind a
    setter runs at the bank's value beside its neighbour on the same bin, and so does the one that reuses a slot."""
    case = debounce_case()
    raw, deb = case.outs[0]["raw"], case.outs[0]["deb"]
    sets = case.outs[0]["sets"]
    assert sorted(e - a for a, e in case.spans)[0] == 1, "one batch is a single frame"
    for f, _, v, states in sets:
        live = case.live(0, f - 1, f)
        assert any(raw[f - 2, l] == raw[f - 1, l] == raw[f, l] == 1 for l in live), f"no mark runs across frame {f}"
        if v == 70:
            assert any(5 <= states[l][3] < 70 and states[l][0] == 5 for l in live), "no count of 5 - 69 at the 70"
            assert states[gen.DEB_FRESH][0] == 1 and case.life[0][gen.DEB_GONE][1] == f
    assert case.refs[0].debouncer_state(gen.DEB_GONE)[0] == 5, "the detached listener is passed by"
    assert case.slot[0][gen.DEB_FRESH] == 70 and case.slot[0][gen.DEB_REUSE] == case.slot[0][gen.DEB_GONE] == gen.DEB_GONE
    upper = [l for l in range(64, gen.DEB_LISTENERS) if not np.array_equal(raw[:, l], deb[:, l])]
    assert len(upper) >= 4, upper
    # the late ones: at the bank's 1 (a pass-through) until a setter reaches them, beside a neighbour on their bin that is not
    for late, twin in ((gen.DEB_FRESH, 1), (gen.DEB_REUSE, 0)):
        start, end, own = listener_sets(case, late)
        assert case.bins[0][late] == case.bins[0][twin] and own
        a, e = start, own[0][0]
        assert np.array_equal(deb[a:e, late], raw[a:e, late]) and not np.array_equal(deb[a:e, twin], raw[a:e, twin]), late
        assert not np.array_equal(deb[e:, late], raw[e:, late]), f"listener {late}: the next setter changes nothing"


def min_window(psd, edge):
    """dsp.FindNoiseFloor's loop (dsp/fft.go:215-243): the bins [from, to) of the window it settles on, and how many windows
    it evaluates."""
    size = (len(psd) - 2 * edge) // 10
    count, total, first, best, at, windows = 0, 0.0, True, float(psd[0]), 0, 0
    for i in range(edge, len(psd) - edge):
        if count == size:
            count, mean, windows = 0, total / size, windows + 1
            if mean < best or first:
                best, first, at = mean, False, i
            total = 0.0
        total += float(psd[i])
        count += 1
    return at - size, at, windows


def test_edge_sequence_moves_the_noise_geometry():
    """Nine- and ten-window geometries both occur; behind every setter some frame's minimum window lies elsewhere in the
    spectrum than the width before would have put it; a setter falls in mid-cumulation, a batch completes two
    cumulations, and a cumulation that spans a setter has peaks."""
    case = gen.case_edge()
    case.run_oracle()
    out = case.outs[0]
    frames = case.oracle_input(0)
    widths = [gen.EDGE] + [v for _, name, v, _ in out["sets"] if name == "edge_width"]
    assert widths == [gen.EDGE] + gen.edge_sequence(gen.N)
    counts = set()
    setters = [f for f, _, _, _ in out["sets"]]
    for f, old, new in zip(setters, widths, widths[1:]):
        moved = 0
        for g in range(f, f + 25):
            psd = orc.iq_to_spectrum_and_psd(frames[g])[1]
            a, b = min_window(psd, old), min_window(psd, new)
            counts.add(b[2])
            assert np.float32(psd[b[0]:b[1]].astype(np.float64).sum() / (b[1] - b[0])) == out["frames"]["min_mean"][g], (g, new)
            moved += a[1] <= b[0] or b[1] <= a[0]
        assert moved >= 1, f"widths {old} and {new} settle on overlapping windows in every frame looked at"
    assert counts == {9, 10}, counts
    assert any(f % 100 for f in setters), "no setter in mid-cumulation"
    assert any(e // 100 - a // 100 >= 2 for a, e in case.spans), "no batch completes two cumulations"
    spanning = [c for c, pf in enumerate(out["peak_frames"]) if any(pf - 99 < f <= pf for f in setters)]
    assert any(len(out["peaks"][c]) > 0 for c in spanning), spanning


def test_peak_thresholds_change_the_peak_lists():
    """Every change of a band's peak threshold changes at least one completed cumulation's peak list from what the threshold
    before would have given (the row, the completing frame's noise floor and dsp.FindPeaks from the oracle); the search is
    off for one cumulation; at +Inf nothing is found."""
    case = gen.case_peaks()
    case.run_oracle()
    for b in range(2):
        out = case.outs[b]
        sets = [(f, v) for f, name, v, _ in out["sets"] if name == "peak_threshold"]
        assert len(sets) >= 2 and all(f % 100 for f, _ in sets), sets
        values = [gen.PEAK_START[b]] + [v for _, v in sets]
        ends = [f for f, _ in sets[1:]] + [case.total]
        off = [(f, v) for f, name, v, _ in out["sets"] if name == "find_peaks"]
        for (f, v), before, end in zip(sets, values, ends):
            changed = 0
            for c, pf in enumerate(out["peak_frames"]):
                if not f <= pf < end or any(lo <= pf < hi for (lo, _), (hi, _) in zip(off[0::2], off[1::2])):
                    continue
                thr = np.float32(before) + out["frames"]["noise_floor"][pf]
                then = orc.find_peaks(out["cumulation"][c], thr, case.rate, case.centers[b])
                now = orc.find_peaks(out["cumulation"][c], out["frames"]["peak_thr"][pf], case.rate, case.centers[b])
                assert now == out["peaks"][c]
                changed += then != now
            assert changed >= 1, f"band {b}: {before} -> {v} at frame {f} changes no peak list"
        searched_off = [c for c, pf in enumerate(out["peak_frames"]) if off[0][0] <= pf < off[1][0]]
        assert len(searched_off) == 1 and out["peaks"][searched_off[0]] == []
        assert values[-1] == float("inf") and out["peaks"][-1] == [] and np.isinf(out["frames"]["peak_thr"][-1])
    assert {v for b in range(2) for _, name, v, _ in case.outs[b]["sets"] if name == "peak_threshold"} == {9.0, 21.5, 0.0, -3.0, float("inf")}
