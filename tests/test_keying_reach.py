"""What the inputs of tests/test_keying_gpu.py reach in k_listen_decode, from the CPU oracle alone: orc.Receiver over each
case's input, orc.Decoder ticked over the debounced bits and read behind every tick (keying_gen.anatomy).  The GPU tests
compare the kernel with the oracle on these very inputs (tests/keying_gen.py holds the table both sides read); a later edit
of the generator, a seed or a step that takes a case off the path it is there for fails here, without a GPU."""
import functools

import numpy as np

import keying_gen as gen
from oracle import oracle as orc

GROUP, ROUND = 16, 32  # k_listen.hip: listener slots per workgroup, edges per round


@functools.lru_cache(maxsize=None)
def base():
    """Case (a) with its oracle run, and every listener's anatomy: {slot: (band, listener, first frame, anatomy)}."""
    case = gen.case_a()
    case.run_oracle()
    who = {}
    for b in range(case.n_bands):
        for lid in range(len(case.bins[b])):
            start = case.life[b][lid][0]
            who[b * case.max_listeners + lid] = (b, lid, start, gen.anatomy(case.outs[b]["deb"][:, lid], case.rate, case.step, start))
    return case, who


def batch_of(case, frame):
    return next(k for k, (a, e) in enumerate(case.spans) if a <= frame < e)


def edges_in(an, a, e):
    return [x for x in an["edges"] if a <= x[0] < e]


def test_base_rounds_and_groups():
    """Six rounds and more (both ring indices wrap) beside an idle listener and one with less than a round, in one workgroup
    and batch; the two batches cut by the oracle's edges hold exactly 64 and 33 edges of the cut listener."""
    case, who = base()
    assert case.n_bands * case.max_listeners == 38 and sorted(who) == list(range(38))
    found = []
    for k, (a, e) in enumerate(case.spans):
        for g0 in range(0, 38, GROUP):
            counts = [len(edges_in(who[s][3], a, e)) for s in range(g0, min(g0 + GROUP, 38)) if who[s][2] < e]
            if max(counts) >= 161 and 0 in counts and any(1 <= c <= 31 for c in counts):
                found.append((k, g0 // GROUP))
    assert {g for _, g in found} == {0, 1, 2}, f"(batch, workgroup) with 6 rounds beside 0 and 1 - 31 edges: {found}"
    b, lid = gen.A_CUT_LISTENER
    an = who[b * case.max_listeners + lid][3]
    assert [len(edges_in(an, *case.spans[k])) for k in (5, 6)] == [64, 33]
    assert case.spans[6][0] in [x[0] for x in an["edges"]], "the batch behind the 64 edges begins with an edge"
    assert [e - a for a, e in case.spans[:5]] == [1024, 1, 63, 64, 65] and sum(e - a == 1024 for a, e in case.spans) >= 3
    # the late listener: until its attach its half-wave partner (slot 19) works alone, then both do
    late = who[gen.A_LATE]
    assert late[2] == case.spans[7][0] and len(late[3]["edges"]) >= 100 and len(who[gen.A_LATE + 1][3]["edges"]) > 0
    for g0 in range(0, 38, GROUP):
        kinds = {(gen.a_kinds(0) + gen.a_kinds(1))[s] for s in range(g0, min(g0 + GROUP, 38))}
        assert kinds >= {"fast", "dahs", "silent", "sparse"}, (g0, kinds)


def test_base_runes():
    """The runes the hostile timing makes, over all 38 listeners."""
    case, who = base()
    overlong = spaces = ninth = aborts = later = later_first = three = 0
    for b, lid, start, an in who.values():
        frames = {x[0]: x for x in an["edges"]}
        edge_at = np.array(sorted(frames), np.int64)
        invalid_at = np.array([x[0] for x in an["edges"] if x[3]], np.int64)
        prev_write = start - 1
        spaces += sum(r == " " for _, r in an["runes"])
        for i, (f, r) in enumerate(an["runes"]):
            if r == "\xa6" and np.any((invalid_at > prev_write) & (invalid_at <= f)):
                overlong += 1  # an over-long mark lies between the last written character and this one
            if r != " ":
                prev_write = f
            if f in frames:
                ninth += frames[f][1] == 0  # a falling edge writes only when a ninth symbol closes the character
                continue
            aborts += 1  # written at a tick that is no edge: the abort check
            began = int(edge_at[edge_at < f][-1]) if np.any(edge_at < f) else start
            k = batch_of(case, f)
            if batch_of(case, began) < k:
                later += 1
                later_first += not np.any((edge_at >= case.spans[k][0]) & (edge_at < f))
        # a rising edge that writes a character and a space; the run behind the next falling edge writes an abort rune
        at = [f for f, _ in an["runes"]]
        for i in range(len(at) - 1):
            f = at[i]
            if f in frames and frames[f][1] == 1 and at[i + 1] == f and an["runes"][i + 1][1] == " ":
                nxt = edge_at[edge_at > f]
                if len(nxt) >= 1:
                    lo, hi = int(nxt[0]), int(nxt[1]) if len(nxt) > 1 else case.total
                    three += any(lo < g < hi for g in at)
    assert overlong >= 50, overlong
    assert spaces >= 50, spaces
    assert ninth >= 5, ninth
    assert aborts >= 20 and later >= 3 and later_first >= 1, (aborts, later, later_first)
    assert three >= 1, three


def test_base_das_and_speeds():
    """More than eight das in one round of 32 edges (a second pass of the speed loop); final speeds from 12 to 40 WPM."""
    case, who = base()
    most = 0
    for b, lid, start, an in who.values():
        for a, e in case.spans:
            ed = edges_in(an, a, e)
            most = max([most] + [sum(x[5] for x in ed[i:i + ROUND]) for i in range(0, len(ed), ROUND)])
    assert most >= 9, most
    wpm = [an["wpm"] for _, _, _, an in who.values()]
    assert min(wpm) <= 12 and max(wpm) >= 40, (min(wpm), max(wpm))


def test_debounce_rows():
    """(b): the debounced bits differ from the raw ones everywhere; in the 4200-frame batch a restart at frame 4094 or 4095
    is carried into word 64 (the count has not reached 3 there), and the state carried into it is up for one listener and
    down for another."""
    assert [d for d, _ in gen.B_ROWS] == [2, 3, 5, 9, 70, 3] and gen.B_ROWS[gen.B_LONG][1] == (4200,)
    for row in range(len(gen.B_ROWS)):
        case = gen.case_b(row)
        case.run_oracle()
        raw, deb = case.outs[0]["raw"], case.outs[0]["deb"]
        assert int((raw != deb).sum()) >= 300, (row, int((raw != deb).sum()))
        # (a debounce of 70 passes only the over-long marks and the noise kind's rare long runs: an edge per listener; the
        # others hundreds)
        assert case.oracle_counts()[0] >= 12 * (1 if case.debounce == 70 else 20), (row, case.oracle_counts())
        if row == gen.B_LONG:
            restart = [lid for lid in range(raw.shape[1]) if raw[4095, lid] != raw[4094, lid] or raw[4094, lid] != raw[4093, lid]]
            assert restart, "no raw change at frame 4094 or 4095"
            assert {int(x) for x in deb[4095]} == {0, 1}, "the state carried into word 64"
            assert any(len(gen.edge_frames(deb[4096:, lid])) > 5 for lid in restart)


def test_deferred_rows():
    """(c): every sdr_attach_at frame lies inside a mark, or in a gap of at most three frames between two marks (inside a
    character), of a carrier that was keyed before."""
    band = gen.c_band()
    deb = gen.oracle_bits(gen.N, gen.RATE, band[0], band[2])
    for i, at in gen.C_LATE:
        f = gen.C_STEPS[0] + at
        ed = gen.edge_frames(deb[:, i])
        assert len(ed[ed < f]) >= 20 and len(ed[ed > f]) >= 2 or at == gen.C_STEPS[1] - 1, (i, at)
        before = int(ed[ed <= f][-1])
        after = int(ed[ed > f][0]) if np.any(ed > f) else None
        assert deb[f, i] == 1 or (after is not None and after - before <= 3), (i, at, before, after)
    assert gen.C_KINDS[0] == gen.C_KINDS[2] == "fast" and gen.C_KINDS[1] == "long"
    assert [at for _, at in gen.C_LATE] == [64, 130, gen.C_STEPS[1] - 1]


def test_other_schedules():
    """(d): the graph row and the overlapped row key and decode: edges and runes on every keyed listener."""
    for case, kinds in ((gen.case_d_graph(), gen.D_KINDS), (gen.case_d_hop(), gen.D_HOP_KINDS)):
        case.run_oracle()
        for lid, kind in enumerate(kinds):
            text = case.decs[0][lid][0]
            edges = len(gen.edge_frames(case.outs[0]["deb"][gen.LEAD:, lid]))  # (behind the chatter of the filling means)
            assert edges == 0 if kind == "silent" else edges >= (1 if kind == "sparse" else 20), (case.path, lid, kind, edges)
            assert kind in ("silent", "sparse", "noise") or len(text) >= 3, (case.path, lid, kind, text)
    assert case.step == gen.D_HOP_N // 4


def test_stop_adds_a_rune():
    """(e): at both cuts Decoder.stop() writes the pending character: "a" at the first, the invalid one at the second."""
    band, cuts = gen.e_input()
    deb = gen.oracle_bits(gen.N, gen.RATE, band[0], band[2])
    for cut, want in zip(cuts, ("a", "\xa6")):
        d = orc.Decoder(gen.RATE, gen.N)
        d.reset()
        d.ticks(deb[:cut, 0])
        before = d.text()
        d.stop()
        assert d.text() == before + want, (cut, before, d.text())
        assert deb[cut - 1, 0] == 0 and deb[cut - 3, 0] == 1, "the cut lies two frames behind a mark"
    assert np.all(deb[cuts[1] - 62:cuts[1] - 2, 0] == 1), "the invalid character's last mark is the over-long one"


def test_text_capacity_overflows():
    """(f): by the oracle every fast listener writes at least 100 runes more than its buffer holds, the clean one fewer than it
    holds, and the batch in which a listener reaches the capacity holds more runes than the room that was left."""
    band, batches, decs = gen.f_input()
    assert band[0].shape[0] == batches * gen.F_BATCH
    for kind, (text, at) in zip(gen.F_KINDS, decs):
        if kind != "fast":
            assert 100 <= len(text) < gen.TEXT_CAP, (kind, len(text))
            continue
        assert len(text) >= gen.TEXT_CAP + gen.F_OVER, len(text)
        k = int(at[gen.TEXT_CAP - 1]) // gen.F_BATCH  # the batch that writes the buffer's last rune
        room = gen.TEXT_CAP - int(np.searchsorted(at, k * gen.F_BATCH))
        held = int(np.searchsorted(at, (k + 1) * gen.F_BATCH)) - int(np.searchsorted(at, k * gen.F_BATCH))
        assert held > room > 0, (k, room, held)
    need = [int(at[gen.TEXT_CAP + gen.F_OVER - 1]) // gen.F_BATCH + 1 for kind, (_, at) in zip(gen.F_KINDS, decs) if kind == "fast"]
    assert batches == max(need), (batches, need)
