"""What the inputs of tests/test_frame_origin_gpu.py reach, from the CPU oracle alone: every case that crosses a multiple of
2^31 has a listener with an edge and a rune strictly in front of the crossing and an edge and a rune at or behind it, the
cuts fall where the table says, and the frame arithmetic of the drivers is what the header says.  A later edit of a
generator, a seed or a step that takes a case off its crossing fails here, without a GPU."""
import numpy as np
import pytest

import frame_origin_gen as fo
import keying_gen as gen
from parity_tools import decode, frames32

CASES = dict(fo.crossing_cases())


def sides(case):
    """Per listener that is never detached: (band, listener, edges before, runes before, edges from, runes from the crossing)."""
    case.run_oracle()
    c = fo.crossing(case.first_frame)
    out = []
    for b in range(case.n_bands):
        for lid, (start, gone) in enumerate(case.life[b]):
            if gone is not None:
                continue
            deb = case.outs[b]["deb"][:, lid]
            ed = gen.edge_frames(deb)
            at = case.decs[b][lid][2] if case.timed else decode(deb[start:], case.rate, case.step)[2] + start
            out.append((b, lid, int((ed < c).sum()), int((at < c).sum()), int((ed >= c).sum()), int((at >= c).sum())))
    return out


def test_origins():
    assert [fo.crossing(o) for o in fo.ORIGINS] == [48, 96, 80]
    assert fo.O31 + 48 == 2 ** 31 and fo.O32 + 96 == 2 ** 32 and fo.O5 + 80 == 5 * 2 ** 32
    assert all(o % 100 == 0 for o in fo.ORIGINS)
    assert fo.cuts(fo.O31, "on")[:3] == (48, 1, 151) and fo.cuts(fo.O31, "in")[:2] == (37, 200)
    # what the 32-bit fields hold: the last frame in front of 2^32 and the first behind it
    assert list(frames32([95, 96], fo.O32)) == [2 ** 32 - 1, 0] and list(frames32([47, 48], fo.O31)) == [2 ** 31 - 1, 2 ** 31]
    assert list(frames32([79, 80], fo.O5)) == [2 ** 32 - 1, 0]


@pytest.mark.parametrize("name", list(CASES))
def test_both_sides_of_the_crossing(name):
    case = CASES[name]
    c = fo.crossing(case.first_frame)
    assert 0 < c < case.total
    rows = sides(case)
    both = [r for r in rows if min(r[2:]) >= 1]
    assert both, f"{name}: no listener with an edge and a rune on both sides of frame {c}: {rows}"
    assert case.oracle_counts()[1] > 0, "no peak"


def test_cuts_and_late_listeners():
    for origin in fo.ORIGINS:
        c = fo.crossing(origin)
        on, inside = fo.eager(origin, "on", 1), fo.eager(origin, "in", 1)
        assert on.spans[0] == (0, c) and on.spans[1] == (c, c + 1)
        a, e = inside.spans[1]
        assert a < c < e and (c - a) % 64 != 0
        # the idle listener on the noise bin is carried across: it exists, and the oracle hears nothing on it behind the burst
        on.run_oracle()
        assert not on.outs[0]["deb"][fo.BURST + 5:, len(on.init_bins[0]) - 1].any()
    for case in (fo.deferred(fo.O31), fo.deferred(fo.O32, wide=True)):
        c = fo.crossing(case.first_frame)
        a, e = case.spans[1]
        assert a < c < e
        for band in range(case.n_bands):
            assert [s for s, _ in case.life[band][3:]] == [c - 5, c, c + 7, e]
    case = fo.graph(fo.O32, False)
    assert [a for a, _ in case.spans] == [0, 40, 80, 120, 160, 200] and fo.crossing(fo.O32) == 96
    case = fo.overlapped(fo.O32)
    assert case.spans[0][0] < 96 < case.spans[0][1] and case.step == fo.HOP
    case = fo.attach_detach(fo.O31)
    assert case.slot[0] == [0, 1, 2, 3, 4, 2, 5] and case.heir[0][2] == 5 and case.life[0][5][0] == 48 and case.life[0][4][0] == 32


def test_the_stop_writes_a_rune_behind_the_crossing():
    case = fo.stop(fo.O32)
    case.run_oracle()
    cut = fo.stop_cut()
    assert cut > 150 and case.stops == {(0, 0): [cut]}
    at = case.decs[0][0][2]
    plain = decode(case.outs[0]["deb"][:, 0], case.rate, case.step)[2]
    assert (at == cut - 1).sum() == (plain == cut - 1).sum() + 1, "the stop adds one rune, stamped with the frame in front of it"
