"""What the default seeds of tests/test_nb_fuzz_gpu.py reach, proved without a GPU: all 42 pairs of the six integer formats
and B = 64 .. 4096, so every bgl = log2(block bytes / 16) from 2 to 10 of every power-kernel base and all three reductions
of k_nb_power; W = 1, 2, 8 and the largest legal one, 64 among them; every class of hold, the ones above 256 samples and
above a wave's 4 KB with planted impulses; ratio_q4 16, 16384 and between; every stream kind, cut, entry point, threshold
event and first sample; and the reference alone, run over every seed, agrees with itself along the cuts and shows that the
stream is informative: at least one impulse, more blanked samples than impulses where hold > 0, 5 % to 70 % of the judged
samples blanked, exactly one impulse in the constant kind - whose one gate of at most B + 1 samples cannot reach 5 % of two
tiles, so that kind is held to its own condition instead - and a saturated threshold in the loud kind."""
import numpy as np
import pytest

import nb_fuzz_gen as gen
import nb_ref as N
from parity_tools import bits_equal


@pytest.fixture(scope="module")
def seeds():
    return gen.seeds()


def base(fmt):
    return fmt & ~N.REAL


def test_default_seeds_reach_every_format_with_every_block_size(seeds):
    assert len(seeds) == gen.DEFAULT_SEEDS == 42
    assert {(s.fmt, s.B) for s in seeds} == {(f, b) for f in N.FORMATS for b in gen.BLOCKS} and gen.BLOCKS == tuple(64 << i for i in range(7))
    for s in seeds:
        assert s.bgl == int(np.log2(s.B * s.sb // 16)) and s.tile * s.sb == 16384 and s.tile_blocks * s.B == s.tile
        assert s.regime == ("segment" if s.bgl < 6 else "rows" if s.bgl <= 7 else "wave")
    # k_nb_power<BASE> at every block size it can meet, k_nb_gate<FMT> at every bgl it can meet
    assert {(base(s.fmt), s.bgl) for s in seeds} == {(N.SC16, b) for b in range(3, 11)} | {(f, b) for f in (N.CS8, N.CU8) for b in range(2, 10)}
    assert {(base(s.fmt), s.bgl) for s in seeds if not N.is_real(s.fmt)} == {(N.SC16, b) for b in range(4, 11)} | {(f, b) for f in (N.CS8, N.CU8) for b in range(3, 10)}
    assert {s.regime for s in seeds} == {"segment", "rows", "wave"}
    for f in N.FORMATS:
        assert {s.regime for s in seeds if s.fmt == f} == {"segment", "rows", "wave"}, f
    for kind in ("wild", "planted"):
        assert {s.regime for s in seeds if s.kind == kind} == {"segment", "rows", "wave"}, kind
    assert any(s.kind == "planted" and s.bgl == 10 for s in seeds)  # a block is the whole tile
    assert len({s.ident for s in seeds}) == len(seeds)


def test_default_seeds_reach_every_window_hold_ratio_and_kind(seeds):
    for s in seeds:
        assert s.W in gen.windows(s.B) and s.W * s.B <= gen.MAX_SPAN and 0 <= s.hold <= s.B and 16 <= s.ratio_q4 <= 16384
        assert s.hold_classes == gen.hold_classes(s.hold, s.B, s.fmt)
    assert {s.W for s in seeds} >= {1, 2, 8, 64}
    assert any(s.W == 65536 // s.B < 64 for s in seeds)  # the largest legal one where B * 64 is too much
    assert set().union(*(s.hold_classes for s in seeds)) == set(gen.HOLD_CLASSES)
    planted = [s for s in seeds if s.kind == "planted"]
    assert set().union(*(s.hold_classes for s in planted)) == set(gen.HOLD_CLASSES)
    # a gate longer than 256 samples, and one longer than a wave's 4 KB, that is not simply B
    assert any("loop" in s.hold_classes and s.hold < s.B for s in planted) and any("wave" in s.hold_classes and s.hold < s.B for s in planted)
    assert any(s.hold > 256 and s.tile_blocks > 1 for s in planted)  # the lookback in front of a tile loops
    ratios = {s.ratio_q4 for s in seeds}
    assert {16, 16384} <= ratios and len(ratios - {16, 16384}) >= 5
    assert {s.kind for s in seeds} == set(gen.KINDS)
    assert {s.fmt for s in seeds if s.kind == "loud"} == {N.SC16, N.RS16}
    for kind in ("wild", "planted", "constant"):
        assert {base(s.fmt) for s in seeds if s.kind == kind} == {N.SC16, N.CS8, N.CU8}, kind
        assert {N.is_real(s.fmt) for s in seeds if s.kind == kind} == {False, True}, kind
    assert all(s.ratio_q4 == 16 for s in seeds if s.kind == "constant") and all(s.ratio_q4 >= 64 for s in seeds if s.kind in ("planted", "loud"))
    assert all(s.ratio_q4 < 48 and s.hold <= 5 for s in seeds if s.kind == "wild")


def test_default_seeds_reach_every_cut_and_event(seeds):
    for s in seeds:
        cuts, tb, W = s.cuts, s.tile_blocks, s.W
        assert sum(cuts) == s.blocks and min(cuts) >= 1 and len(s.entries) == len(s.thresholds) == len(cuts)
        # two whole tiles, a part tile (where a tile is more than a block) and a block behind the W unjudged blocks
        assert s.blocks - W >= 2 * tb + 2 and (tb == 1 or s.blocks % tb != 0) and s.n == s.blocks * s.B
        assert 1 in cuts and tb in cuts and tb + 1 in cuts
        if W >= 2:  # a run of calls with fewer than W blocks in all
            assert any(sum(cuts[i:j]) < W for i in range(len(cuts)) for j in range(i + (1 if W == 2 else 2), len(cuts) + 1)), s.ident
        x = s.long_call
        assert cuts[x] == 2 and cuts[x + 1] == 1 and sum(cuts[:x]) >= W
        assert s.thresholds[x] == (s.ratio_q4, s.B) and s.thresholds[x + 1] == (s.ratio_q4, 1)
        assert x + 2 >= len(cuts) or s.thresholds[x + 2] == (s.ratio_q4, s.hold)
        if s.off_at is not None:
            assert s.thresholds[s.off_at] == (0, s.hold) and s.thresholds[s.off_at + 1] == (s.ratio_q4, s.hold)
        assert s.first % s.B == 0 and s.first >= 0 and all(0 <= r < len(cuts) - 1 for r in s.reads)
    assert sum(s.off_at is not None for s in seeds) >= 40
    assert {e for s in seeds for e in s.entries} == {"device", "host"} == {s.whole_entry for s in seeds}
    assert any(len(set(s.entries)) == 2 for s in seeds)
    assert {len(s.reads) for s in seeds} == {0, 1, 2}
    assert {s.first_kind for s in seeds} == set(gen.FIRSTS)
    big = [s for s in seeds if s.first_kind == "2^32"]
    assert all(s.first > 1 << 32 and (s.first // s.B) % 2 == 1 for s in big) and {base(s.fmt) for s in big} >= {N.CU8}
    # the planted kind: every structure's last and first sample, in the whole stream's geometry and in a call's
    planted = [s for s in seeds if s.kind == "planted"]
    whats = {"window", "long", "call", "tile", "wave", "row", "group", "block", "call-tile", "call-wave", "call-row", "call-group", "single"}
    assert set().union(*(set(s.plants) for s in planted)) == whats
    for s in planted:
        assert {"window", "long", "call", "tile", "wave", "row", "group", "block"} <= set(s.plants), s.ident
        assert s.plants["window"] == [s.W * s.B - 1, s.W * s.B]
        end = (sum(s.cuts[:s.long_call]) + 2) * s.B
        assert s.plants["long"] == [end - 2] and s.plants["call"][:2] == [end - 1, end]
        for what, size in (("tile", s.tile), ("wave", 4096 // s.sb), ("row", 1024 // s.sb), ("group", 16 // s.sb), ("block", s.B)):
            p = s.plants[what]  # a structure's last sample and, at another boundary where there is one, a structure's first
            assert len(p) == 2 and (p[0] + 1) % size == 0 and p[1] % size == 0 and min(p) > s.W * s.B, (s.ident, what)
    assert all(not s.plants for s in seeds if s.kind != "planted")


@pytest.mark.parametrize("seed", gen.seeds(), ids=lambda s: s.ident)
def test_the_reference_alone(seed):
    s = seed
    raw = s.raw()
    assert raw.dtype == N.RAW_DTYPE[s.fmt] and raw.shape == ((s.n,) if N.is_real(s.fmt) else (s.n, 2))
    assert bits_equal(raw, s.raw())
    (whole, stats), (outs, reads) = s.reference(raw)
    judged = s.n - s.W * s.B
    print(s.ident, stats, "judged", judged)
    assert stats["samples"] == s.n and bits_equal(whole[:s.W * s.B], raw[:s.W * s.B])
    # cut and whole agree when no threshold changes
    plain, plain_reads = s.reference_cut(raw, thresholds=False)
    assert bits_equal(np.concatenate(plain), whole)
    total = plain_reads[0]
    for r in plain_reads[1:]:
        total = N.add_stats(total, r)
    assert total == stats and len(plain_reads) == len(s.reads) + 1 == len(reads)
    assert sum(r["samples"] for r in reads) == s.n and [len(o) for o in outs] == [c * s.B for c in s.cuts]
    # the stream is informative
    assert stats["impulses"] >= 1
    assert s.hold == 0 or stats["blanked"] > stats["impulses"]
    assert stats["blanked"] >= stats["impulses"]
    changed = (whole != raw).reshape(s.n, -1).any(axis=1)
    if s.kind == "constant":
        # m * span * 16 == ratio_q4 * R in every block judged against unchanged blocks; the one larger sample is the impulse
        m = N.mags(raw, s.fmt)
        assert stats["impulses"] == 1 and stats["blanked"] == min(s.hold + 1, s.n - s.bump)
        assert len(set(np.delete(m, s.bump))) == 1 and m[s.bump] > m[0] and changed[s.bump] and s.bump >= s.W * s.B
        p = int(m[:s.B].sum())
        assert int(m[0]) * s.B * s.W * 16 == s.ratio_q4 * p * s.W and m[0] > 0
    else:
        assert 0.05 * judged <= stats["blanked"] <= 0.70 * judged, stats["blanked"] / judged
    thr = s.block_thresholds(raw)
    assert thr[:s.W] == [None] * s.W and all(t is not None for t in thr[s.W:])
    if s.kind == "loud":
        # a saturated threshold: the quotient itself, not "off" or "not judged"; and a full-scale sample there is not blanked
        sat = [j for j, t in enumerate(thr) if t == gen.NEVER]
        assert len(sat) >= 2 and s.ratio_q4 != 0
        full = np.asarray(raw[sat[0] * s.B:(sat[0] + 1) * s.B] == np.asarray(N.full_scale(s.fmt), raw.dtype)).reshape(s.B, -1).all(axis=1)
        assert full.all() and not changed[sat[0] * s.B + s.hold + 1:(sat[0] + 1) * s.B].any()
        # one full-scale sample after W quiet blocks is caught
        single = (2 * s.W + 2 + s.W) * s.B
        at = single + int(np.flatnonzero(N.mags(raw[single:single + s.B], s.fmt) == N.mags(raw[s.W * s.B:s.W * s.B + 1], s.fmt)[0])[0])
        assert changed[at] and not changed[at - 1]
    else:
        assert all(t < gen.NEVER for t in thr[s.W:])
    if s.kind == "planted":
        # block W - 1's last sample is not judged, block W's first is; the long gate covers the whole call behind the
        # long-hold call although that call's own hold is 1
        w = s.W * s.B
        assert not changed[w - 1] and changed[w]
        x = s.long_call
        at = s.first + sum(s.cuts[:x + 1]) * s.B
        assert bits_equal(outs[x + 1], N.blank_words(at + np.arange(s.B), s.fmt)), "the gate of B samples does not cover the next call"
        noise = np.ones(s.n, bool)
        noise[[p for v in s.plants.values() for p in v]] = False
        assert stats["impulses"] <= (~noise).sum() and stats["impulses"] >= 0.5 * (~noise[w:]).sum()  # no noise sample is an impulse
