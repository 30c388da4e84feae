"""The seeded generator of tests/test_nb_fuzz_gpu.py (pure NumPy: tests/test_nb_fuzz_coverage.py runs it without a GPU and
proves what the default seeds reach).

The blanker's two streaming kernels (csrc/k_nb.hip) own tiles of 16 KB of raw bytes - four waves of 4 KB, each four rows of
1 KB, a lane 16 bytes - and branch on bgl = log2(block bytes / 16), 2 .. 10: the power kernel reduces within a row's segment
(bgl < 6), over one or two whole rows (6, 7) or over a wave's four rows (>= 8), the gate kernel indexes its thresholds with
it.  A seed draws
  the format and B   the first 42 seeds walk the six integer formats x B = 64, 128 .. 4096: every bgl of every power-kernel
                     base and every gate instantiation; later seeds draw both;
  W                  from 1, 2, 8 and the largest legal one, min(64, 65536 / B);
  hold               by class (hold_classes): 0, 1, B, above the samples of a 16-byte group, above 256 (the lookback in
                     front of a tile runs more than once per thread) and above the samples of a wave's 4 KB (a gate crosses
                     waves), the last two where B allows them;
  ratio_q4           16, 16384 or between, within what the kind allows (below);
  the stream kind    "wild"      whole-range random words, ratio 1.5 .. 2.5 and hold <= 5 (_WILD)
                     "planted"   a few LSB of noise (nb_ref.random_raw with a spread) and full-scale samples at the last
                                 sample of one and the first sample of another of every structure - 16-byte group, 1 KB row,
                                 4 KB wave part, 16 KB tile, block and call, in the whole stream's geometry and in a long
                                 call's (a pair p - 1, p where there is one boundary only, and at call boundaries) - at
                                 the last sample of block W - 1 (not judged) and the first of block W (judged), and two
                                 samples in front of the end of the call that the long-hold event follows; then single ones
                                 at random until an eighth of the judged samples is blanked.  The ratio is at least 4 (the
                                 noise's largest m is three times its mean: no noise sample is an impulse) and at most
                                 8 / the plants' density and 8 B W, so that a plant among plants is still an impulse
                     "constant"  every sample has the same m, and ratio_q4 = 16: m * span * 16 == ratio_q4 * R exactly and
                                 nothing is an impulse (the inequality is strict); one sample is one unit larger and is one
                     "loud"      16-bit formats only (an 8-bit format's quotient stays below 2^28): periods of W + 2
                                 full-scale blocks and 2 W + 1 quiet ones with one full-scale sample in the middle one,
                                 ratio_q4 >= 64: inside a full-scale stretch the threshold's quotient is 2^32 or more and
                                 saturates to "never"; at a stretch's start and after W quiet blocks a full-scale sample
                                 is caught
  length             W unjudged blocks, then at least two tiles, a part tile and a block, and at least 64 gates' worth;
  cuts               in blocks: always a call of one block, a run of calls with fewer than W blocks in all (W >= 2), a call
                     of two blocks with the long-hold event and a call of one block behind it, a call of exactly one tile and
                     one of a tile and a block; the rest drawn;
  per call           the entry point, and in the cut run thresholds in front of calls: (ratio, B) in front of the long-hold
                     call, (ratio, 1) - a shorter hold while that gate is open - in front of the next, the seed's own
                     behind it; off in front of one call and on again in front of the next; reads of the statistics behind
                     drawn calls;
  the first sample   0, a multiple of B, or an odd number of blocks above 2^32.
A plain helper module, not a test file."""
import numpy as np

import nb_ref as N

TILE_BYTES = 16384  # csrc/nb.h kNbTileBytes
WAVE_BYTES, ROW_BYTES, GROUP_BYTES = 4096, 1024, 16
BLOCKS = (64, 128, 256, 512, 1024, 2048, 4096)
DEFAULT_SEEDS = len(N.FORMATS) * len(BLOCKS)
MAX_SPAN = 65536
KINDS = ("wild", "planted", "constant", "loud")
FIRSTS = ("zero", "multiple", "2^32")
HOLD_CLASSES = ("zero", "one", "B", "group", "loop", "wave")
NEVER = 0xFFFFFFFF
_KINDS16 = ("wild", "loud", "planted", "constant")
_KINDS8 = ("planted", "wild", "constant")
# the wild kind: ratio_q4 -> the holds (from, below) with which 5 % to 70 % of whole-range random samples are blanked.  With
# r = ratio_q4 / 16 a real sample is an impulse where x^2 > r / 3 (0.29, 0.18, 0.09 of them at r = 1.5, 2, 2.5), a complex
# one where x^2 + y^2 > 2 r / 3 (0.21, 0.10, 0.017), and a hold h blanks 1 - (1 - p)^(h + 1)
_WILD = {False: {24: (0, 3), 32: (0, 4), 40: (3, 6)}, True: {24: (0, 2), 32: (0, 4), 40: (0, 4)}}


def sample_bytes(fmt):
    return np.dtype(N.RAW_DTYPE[fmt]).itemsize * (1 if N.is_real(fmt) else 2)


def windows(block):
    return (1, 2, 8, min(64, MAX_SPAN // block))


def hold_classes(hold, block, fmt):
    """The classes a hold belongs to; "loop" and "wave" exist only where B is above 256 or above a wave's samples."""
    sb = sample_bytes(fmt)
    c = set()
    if hold == 0:
        c.add("zero")
    if hold == 1:
        c.add("one")
    if hold == block:
        c.add("B")
    if hold > GROUP_BYTES // sb:
        c.add("group")
    if hold > 256:
        c.add("loop")
    if hold > WAVE_BYTES // sb:
        c.add("wave")
    return c


def _draw_hold(rng, cls, block, fmt):
    spg, wave = GROUP_BYTES // sample_bytes(fmt), WAVE_BYTES // sample_bytes(fmt)
    if cls == "zero":
        return 0
    if cls == "one":
        return 1
    if cls == "B":
        return block
    if cls == "group":
        return int(rng.integers(spg + 1, min(block, 2 * spg + 30)))
    if cls == "loop":
        return int(rng.integers(257, block))
    assert cls == "wave" and block > wave + 1
    return int(rng.integers(wave + 1, block))


def _hold_pool(kind, block, fmt):
    wave = WAVE_BYTES // sample_bytes(fmt)
    if kind == "wild":
        return ["zero", "one"]
    pool = ["zero", "one", "B", "group"] + (["loop"] if block > 257 else []) + (["wave"] if block > wave + 1 else [])
    return [c for c in pool if c != "B"] if kind == "loud" else pool


def _table(seed):
    """(format, B, kind) of a default seed: the formats in turn, B from 64 up, the kinds in turn along B."""
    fi, bi = seed % len(N.FORMATS), seed // len(N.FORMATS)
    fmt = N.FORMATS[fi]
    if (fmt & ~N.REAL) == N.SC16:
        return fmt, BLOCKS[bi], _KINDS16[(bi + (0 if fmt == N.SC16 else 2)) % 4]
    return fmt, BLOCKS[bi], _KINDS8[(bi + fi) % 3]


class Seed:
    """Everything one seed draws; raw() makes the stream, reference(raw) what the blanker must deliver."""

    def __init__(self, seed):
        self.seed = seed
        rng = np.random.default_rng(77_000 + seed)
        if seed < DEFAULT_SEEDS:
            fi, bi = seed % len(N.FORMATS), seed // len(N.FORMATS)
            self.fmt, self.B, self.kind = _table(seed)
            self.W = windows(self.B)[(fi + bi + bi // 4) % 4]
            # the classes of hold in turn among the seeds of one kind, the longest first
            pool = _hold_pool(self.kind, self.B, self.fmt)
            cls = pool[::-1][sum(_table(t)[2] == self.kind for t in range(seed)) % len(pool)]
            cls = "wave" if "wave" in pool else cls  # (few pairs allow it)
            self.first_kind = FIRSTS[seed % len(FIRSTS)]
        else:
            self.fmt, self.B = int(rng.choice(N.FORMATS)), int(rng.choice(BLOCKS))
            sixteen = (self.fmt & ~N.REAL) == N.SC16
            self.kind = str(rng.choice(_KINDS16 if sixteen else _KINDS8))
            self.W = int(rng.choice(windows(self.B)))
            cls = str(rng.choice(_hold_pool(self.kind, self.B, self.fmt)))
            self.first_kind = str(rng.choice(FIRSTS))
        fmt, B, W = self.fmt, self.B, self.W
        self.sb = sample_bytes(fmt)
        self.bgl = (B * self.sb // GROUP_BYTES).bit_length() - 1
        self.regime = "segment" if self.bgl < 6 else "rows" if self.bgl < 8 else "wave"
        self.tile = TILE_BYTES // self.sb
        self.tile_blocks = tb = self.tile // B
        assert 2 <= self.bgl <= 10 and tb >= 1 and B * W <= MAX_SPAN
        self.wild_ratio = int(rng.choice(sorted(_WILD[N.is_real(fmt)])))
        self.hold = _draw_hold(rng, cls, B, fmt) if self.kind != "wild" else int(rng.integers(*_WILD[N.is_real(fmt)][self.wild_ratio]))
        self.hold_classes = hold_classes(self.hold, B, fmt)
        # the judged part: two tiles, a part tile and a block at least; 30 gates' worth; two periods of the loud kind
        judged = max(2 * tb + int(rng.integers(1, tb)) if tb > 1 else 3, -(-64 * (self.hold + 2) // B), 2 * (3 * W + 3) if self.kind == "loud" else 0)
        judged = max(judged, 2 * tb + 6) + int(rng.integers(0, 3))  # (room for the calls that are always there)
        if tb > 1 and (W + judged) % tb == 0:
            judged += 1
        self.blocks = W + judged
        self.n = self.blocks * B
        if self.first_kind == "zero":
            self.first = 0
        elif self.first_kind == "multiple":
            self.first = int(rng.integers(1, 1 << 20)) * B
        else:
            self.first = ((1 << 32) // B + 2 * int(rng.integers(1, 1 << 16)) + 1) * B
            assert (self.first // B) % 2 == 1 and self.first > 1 << 32
        self.cuts, self.long_call = self._cuts(rng)
        calls = len(self.cuts)
        self.entries = [str(e) for e in rng.choice(["device", "host"], calls)]
        self.whole_entry = "host" if seed % 2 else "device"
        self.reads = tuple(sorted({int(i) for i in rng.integers(0, calls - 1, int(rng.integers(0, 3)))}))
        self._plan_plants(rng)
        self.bump = int(rng.integers(W * B, self.n)) if self.kind == "constant" else None
        self.ratio_q4 = self._ratio(rng)
        # thresholds in front of the cut run's calls
        x = self.long_call
        self.thresholds = [None] * calls
        self.thresholds[x] = (self.ratio_q4, B)
        self.thresholds[x + 1] = (self.ratio_q4, 1)
        if x + 2 < calls:
            self.thresholds[x + 2] = (self.ratio_q4, self.hold)
        free = [i for i in range(calls - 1) if all(self.thresholds[j] is None for j in (i, i + 1)) and (i + 2 >= calls or self.thresholds[i + 2] is None)]
        judged = [i for i in free if sum(self.cuts[:i]) >= W]  # (off and on again where samples are judged, if there is such a call)
        self.off_at = int(rng.choice(judged or free)) if free else None
        if self.off_at is not None:
            self.thresholds[self.off_at] = (0, self.hold)
            self.thresholds[self.off_at + 1] = (self.ratio_q4, self.hold)
        self.ident = (f"s{seed}-{N.FORMAT_IDS[N.FORMATS.index(fmt)]}-B{B}-W{W}-h{self.hold}-r{self.ratio_q4}-{self.kind}-{self.first_kind}")

    # -- the cuts ----------------------------------------------------------------------------------------------------------
    def _cuts(self, rng):
        """(blocks per call, adding up to self.blocks; the index of the long-hold call, which a call of one block follows)."""
        tb, W, left = self.tile_blocks, self.W, self.blocks
        groups = [("one", [1]), ("long", [2, 1]), ("tile", [tb]), ("tile+", [tb + 1])]
        if W >= 2:
            run = [1] if W == 2 else [1, 2, 1] if W <= 8 else [1, int(rng.integers(2, W // 2)), 1]
            assert sum(run) < W
            groups.append(("short", run))
        left -= sum(sum(g) for _, g in groups)
        assert left >= 0, (self.blocks, groups)
        while left > 0:
            c = min(left, int(rng.choice([1, 2, int(rng.integers(1, tb + 2)), int(rng.integers(1, 2 * tb + 3))])))
            groups.append(("drawn", [c]))
            left -= c
        rng.shuffle(groups)
        # the long-hold call lies behind the W unjudged blocks (the last place always does)
        long = next(g for g in groups if g[0] == "long")
        groups.remove(long)
        behind = [i for i in range(len(groups) + 1) if sum(sum(g) for _, g in groups[:i]) >= W]
        groups.insert(int(rng.choice(behind)), long)
        cuts, long_call = [], None
        for name, g in groups:
            if name == "long":
                long_call = len(cuts)
            cuts += g
        return cuts, long_call

    def call_starts(self):
        return np.cumsum([0] + self.cuts)[:-1] * self.B

    # -- the plants --------------------------------------------------------------------------------------------------------
    def _plan_plants(self, rng):
        """self.plants: {what: [positions]} of the planted kind's full-scale samples (empty for the other kinds)."""
        self.plants = {}
        if self.kind != "planted":
            return
        B, W, n, hold, sb = self.B, self.W, self.n, self.hold, self.sb
        judged0 = W * B
        covered = np.zeros(n + B + 2, bool)
        limit = 0.45 * (n - judged0)

        def add(what, places):
            places = [p for p in places if 0 <= p < n]
            trial = covered.copy()
            for p in places:
                if p >= judged0:
                    trial[p:p + hold + 1] = True
            if trial[judged0:n].sum() > limit:
                return
            covered[:] = trial
            self.plants.setdefault(what, []).extend(places)

        starts = self.call_starts()
        ends = starts + np.array(self.cuts) * B
        add("window", [judged0 - 1, judged0])
        add("long", [int(ends[self.long_call]) - 2])
        add("call", [int(ends[self.long_call]) - 1, int(ends[self.long_call])])
        sizes = (("tile", self.tile), ("wave", WAVE_BYTES // sb), ("row", ROW_BYTES // sb), ("group", GROUP_BYTES // sb), ("block", B))
        # the whole stream's geometry: boundaries counted from sample 0, in the judged part, not on a larger structure's
        for i, (what, size) in enumerate(sizes):
            inside = [p for p in range(size, n, size) if p > judged0 + 1 and (what == "block" or all(p % s for _, s in sizes[:i]))]
            if not inside and what != "block":  # (a block of a tile or more: every boundary is a tile's)
                inside = [p for p in range(size, n, size) if p > judged0 + 1]
            self._plant_ends(rng, add, what, inside)
        # a long call's geometry: boundaries counted from the call's first sample
        longest = int(np.argmax(self.cuts))
        a, e = int(starts[longest]), int(ends[longest])
        for what, size in sizes[:4]:
            inside = [p for p in range(a + size, e, size) if p > judged0 + 1]
            self._plant_ends(rng, add, "call-" + what, inside)
        for i in [i for i in rng.permutation(len(starts)) if starts[i] > judged0 + B][:4]:  # (block W - 1 keeps its one plant)
            add("call", [int(starts[i]) - 1, int(starts[i])])
        # single ones until an eighth of the judged samples is blanked
        want = 0.125 * (n - judged0)
        for p in rng.permutation(np.arange(judged0, n)):
            if covered[judged0:n].sum() >= want:
                break
            add("single", [int(p)])
        self.plant_density = sum(len(v) for v in self.plants.values()) / (n - judged0)

    @staticmethod
    def _plant_ends(rng, add, what, boundaries):
        """The last sample in front of one boundary and the first behind another, where there are two: behind a pair
        p - 1, p the gate is p's, and whether p - 1's was carried across the boundary does not show."""
        if len(boundaries) >= 2:
            p, q = (int(v) for v in rng.choice(boundaries, 2, replace=False))
            add(what, [p - 1])
            add(what, [q])
        elif boundaries:
            add(what, [boundaries[0] - 1, boundaries[0]])

    def _ratio(self, rng):
        if self.kind == "constant":
            return 16
        if self.kind == "wild":
            return self.wild_ratio
        pick = self.seed % 3 if self.seed < DEFAULT_SEEDS else int(rng.integers(0, 3))
        if self.kind == "loud":
            # (W > 2: at ratio / 16 = 4 a stretch's first W / 4 blocks are impulses; at a larger one only the first)
            return [16384, 64, int(rng.integers(64, 16385))][pick] if self.W <= 2 else 64
        noise = 3e-6 if (self.fmt & ~N.REAL) == N.SC16 else 3e-4  # the noise's mean m over the full-scale one
        top = int(min(16384, 8 * self.B * self.W, max(64, 8 / (self.plant_density + noise))))  # (8 B W: one plant in the window)
        return [top, 64, int(rng.integers(64, top + 1))][pick]

    # -- the stream --------------------------------------------------------------------------------------------------------
    def raw(self):
        fmt, n, B, W = self.fmt, self.n, self.B, self.W
        rng = np.random.default_rng(333_000 + self.seed)
        sixteen = (fmt & ~N.REAL) == N.SC16
        quiet = lambda: N.random_raw(n, fmt, 444_000 + self.seed, 100 if sixteen else 3)  # noqa: E731
        if self.kind == "wild":
            return N.random_raw(n, fmt, 444_000 + self.seed)
        if self.kind == "planted":
            x = quiet()
            for places in self.plants.values():
                for p in places:
                    x[p] = N.full_scale(fmt)
            return x
        if self.kind == "loud":
            x = quiet()
            # W + 2 full-scale blocks, W quiet ones, one with a single full-scale sample, W quiet ones; the stream may end
            # inside a period
            period, j = 3 * W + 3, W
            while j < self.blocks:
                x[j * B:(j + W + 2) * B] = N.full_scale(fmt)
                if j + 2 * W + 2 < self.blocks:
                    x[(j + 2 * W + 2) * B + int(rng.integers(0, B))] = N.full_scale(fmt)
                j += period
            return x
        # constant: one m everywhere, the signs and (complex) the order of the two parts drawn
        base = fmt & ~N.REAL
        a, b = (int(v) for v in (rng.integers(1000, 23000, 2) if sixteen else rng.integers(10, 90, 2)))
        word = (lambda u: (u + 255) // 2) if base == N.CU8 else (lambda u: u)  # the raw word of unit u (cu8: u odd)
        if base == N.CU8:
            a, b = a | 1, b | 1
        sign = rng.choice([-1, 1], (n, 2))
        if N.is_real(fmt):
            u = a * sign[:, 0]
        else:
            u = np.where((rng.random(n) < 0.5)[:, None], [a, b], [b, a]) * sign
        x = np.asarray(word(u)).astype(N.RAW_DTYPE[fmt])
        # one unit larger in magnitude (uint8: the next raw word, two units)
        at = self.bump if N.is_real(fmt) else (self.bump, 0)
        x[at] = int(x[at]) + (1 if int(N.units(x[at], fmt)) > 0 else -1)
        return x

    def pieces(self, raw):
        at = np.cumsum([0] + self.cuts) * self.B
        return [raw[a:e] for a, e in zip(at[:-1], at[1:])]

    # -- the reference -----------------------------------------------------------------------------------------------------
    def reference(self, raw):
        """((whole-stream output, its statistics), (the cut run's outputs per call, its reads))."""
        ref = N.NbRef(self.fmt, self.B, self.W, self.ratio_q4, self.hold, self.first)
        whole = (ref.process(raw), ref.read_stats())
        return whole, self.reference_cut(raw)

    def reference_cut(self, raw, thresholds=True):
        ref = N.NbRef(self.fmt, self.B, self.W, self.ratio_q4, self.hold, self.first)
        outs, reads = [], []
        for i, p in enumerate(self.pieces(raw)):
            if thresholds and self.thresholds[i] is not None:
                ref.set_threshold(*self.thresholds[i])
            outs.append(ref.process(p))
            if i in self.reads:
                reads.append(ref.read_stats())
        reads.append(ref.read_stats())
        return outs, reads

    def block_thresholds(self, raw):
        """What csrc/host/nb_rule.h nb_threshold gives each block of the whole stream, in Python integers (None: not judged)."""
        p = [int(v) for v in N.mags(raw, self.fmt).reshape(self.blocks, self.B).sum(axis=1)]
        shift = (self.B * self.W).bit_length() - 1 + 4
        return [None if j < self.W else min(NEVER, (self.ratio_q4 * sum(p[j - self.W:j])) >> shift) for j in range(self.blocks)]


def seeds(n=DEFAULT_SEEDS):
    return [Seed(s) for s in range(n)]
