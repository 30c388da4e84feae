"""The seeded generator of tests/test_ddc_fuzz_gpu.py (pure NumPy: tests/test_ddc_fuzz_coverage.py runs it without a GPU,
checks shape() below against the library's own ddc_shape and proves what the default seeds reach).

The down-converter's kernel (csrc/k_ddc.hip) takes one of nine tile shapes (chunk outputs, threads) by the decimation D and
the tap count T (csrc/ddc.h ddc_shape).  A seed draws
  the input format   one of the four (ddc_ref.FORMATS);
  (D, T)             the first 36 seeds walk TABLE - nine shape classes x four formats, a class's example geometries in
                     turn (where there are two: one with T - 1 well below D * chunk, one with T near 4096); later seeds
                     draw D in 1 .. 256 and T in 1 .. 4096;
  n_bands            from BANDS, lowered where n_bands * T * outputs would exceed COST_CAP (the reference's cost; never
                     the outputs or the shape);
  steps              per band from STEPS or random;
  the first sample   0, a multiple of D, or one that puts 2^31 or 2^32 inside the run;
  cuts               the stream cut into calls, in outputs: always a call of D samples and one of exactly `chunk`
                     outputs, two consecutive calls shorter than T - 1 samples (at most TILE / 4 outputs each) where
                     T - 1 > 2 D, calls of chunk - 1 and chunk + 1 outputs where they still fit, the rest drawn;
  entries            per call "device" or "host" (the whole-stream call: whole_entry);
  retune             optional (call, band, step): sdr_ddc_set_nco_step in front of that call of the cut run;
  switch_at          optional: sdr_ddc_set_stream with a second stream in front of that call of the cut run;
  the value kind     "plain"      the format's whole range (ddc_ref.random_raw)
                     "zeros"      an all-zero stream, for float32 with drawn signs: every output word is +0 (cu8 has no
                                  zero sample and never draws it)
                     "nonfinite"  float32 only: random_raw with the seven PLANTS in single samples, a gap apart - products
                                  that overflow, Inf - Inf, Inf * 0, NaN, -0; at least half of the outputs stay finite
                     "full_scale" the integer formats: random_raw with runs of the type's minimum and maximum.
The stream has 2 * TILE + chunk + 1 outputs per band whatever else is drawn: whole tiles, the short last chunk of a tile,
and a last tile of one whole chunk and one output.

Among the table's seeds the zeros go to the classes of one output per lane only: an all-zero result cannot tell a lane's
two outputs apart, and each of those seeds is meant to notice when they are swapped.  A plain helper module, not a test
file."""
import numpy as np

import ddc_ref as R

TILE = 512          # SDR_DDC_TILE_OUTPUTS
MAX_THREADS = 256   # csrc/ddc.h kDdcMaxThreads
MAX_LDS = 160 * 1024
MAX_D, MAX_T = 256, 4096
DEFAULT_SEEDS = 36
BANDS = (1, 2, 3, 7, 64)
STEPS = (0, 1, -1, 32767, -32768)
FIRSTS = ("zero", "multiple", "2^31", "2^32")
KINDS = ("plain", "zeros", "nonfinite", "full_scale")
COST_CAP = 10 ** 8
FLT_MAX = float(np.finfo(np.float32).max)
PLANTS = ((np.inf, 0.25), (-np.inf, -0.5), (np.nan, 0.1), (FLT_MAX, FLT_MAX), (-FLT_MAX, FLT_MAX), (0.5, np.inf), (-0.0, -0.0))
# (chunk, threads) -> example geometries
TABLE = (
    ((512, 256), ((3, 7),)),
    ((448, 256), ((40, 257), (33, 4096))),
    ((384, 256), ((48, 96), (37, 4095))),
    ((320, 256), ((56, 300), (63, 257))),
    ((256, 256), ((64, 1024), (79, 257))),
    ((192, 192), ((100, 100), (97, 1531))),
    ((128, 128), ((150, 300), (158, 257))),
    ((64, 64), ((256, 4096), (200, 200), (256, 1))),
    ((63, 64), ((255, 4096), (253, 4095))),
)
CLASSES = tuple(c for c, _ in TABLE)


def width(c, d, t):
    return (((c - 1) * d + t + d - 1) // d) | 1


def shape(d, t):
    """(chunk, threads, width, lds_bytes): csrc/ddc.h ddc_shape restated (the coverage test holds it to the header)."""
    c = TILE
    while c > 1 and d * width(c, d, t) * 8 > MAX_LDS:
        c -= 1
    if c >= 64:
        c -= c % 64
    return c, min((c + 63) // 64 * 64, MAX_THREADS), width(c, d, t), d * width(c, d, t) * 8


def _kind(rng, fmt, table_class, d, t, outputs):
    special = "nonfinite" if fmt == R.F32 else "full_scale"
    if table_class is None:
        kind = str(rng.choice(["plain", special] + (["zeros"] if fmt != R.CU8 else [])))
        # (one plant reaches ceil(T / D) outputs: where seven cannot leave half of the outputs finite, the seed is a plain one)
        return "plain" if kind == "nonfinite" and t + len(PLANTS) * d > 45 * outputs * d // 100 else kind
    two_per_lane = CLASSES[table_class][0] > CLASSES[table_class][1]
    pool = ["plain", special] if two_per_lane else ([special, "plain"] if fmt == R.CU8 else ["zeros", special, "plain"])
    return pool[(table_class + fmt) % len(pool)]


class Seed:
    """Everything one seed draws; raw() makes the stream, reference(cos, sin) what the DDC must deliver."""

    def __init__(self, seed):
        self.seed = seed
        rng = np.random.default_rng(88_000 + seed)
        table_class = seed % len(TABLE) if seed < DEFAULT_SEEDS else None
        if table_class is not None:
            self.fmt = R.FORMATS[seed // len(TABLE)]
            examples = TABLE[table_class][1]
            self.d, self.t = examples[self.fmt % len(examples)]
            bands, first = BANDS[seed % len(BANDS)], FIRSTS[seed % len(FIRSTS)]
        else:
            self.fmt = int(rng.choice(R.FORMATS))
            self.d = int(rng.choice([int(rng.integers(1, 9)), int(rng.integers(1, MAX_D + 1)), int(rng.integers(30, MAX_D + 1))]))
            self.t = int(rng.choice([int(rng.integers(1, 65)), int(rng.integers(1, MAX_T + 1)), int(rng.integers(MAX_T - 200, MAX_T + 1))]))
            bands, first = int(rng.choice(BANDS)), str(rng.choice(FIRSTS))
        d, t = self.d, self.t
        self.chunk, self.threads, self.width, self.lds_bytes = shape(d, t)
        self.cls = (self.chunk, self.threads)
        assert table_class is None or self.cls == CLASSES[table_class], (seed, self.cls)
        self.outputs = m = 2 * TILE + self.chunk + 1
        self.n_bands = max(b for b in BANDS if b <= bands and (b == 1 or b * t * m <= COST_CAP))
        self.cost = self.n_bands * t * m
        self.steps = [int(STEPS[i]) if i < len(STEPS) else int(rng.integers(-32768, 32768)) for i in rng.integers(0, len(STEPS) + 1, self.n_bands)]
        self.kind = _kind(rng, self.fmt, table_class, d, t, m)
        self.first_kind = first
        if first == "zero":
            self.first = 0
        elif first == "multiple":
            self.first = int(rng.integers(1, 1 << 20)) * d
        else:  # the edge lies inside the run: first < edge < first + outputs * D
            edge = 2 ** 31 if first == "2^31" else 2 ** 32
            self.first = (edge - int(rng.integers(d, (m - 1) * d + 1))) // d * d
            assert self.first < edge < self.first + m * d
        self.cuts = self._cuts(rng)
        n = len(self.cuts)
        self.entries = [str(e) for e in rng.choice(["device", "host"], n)]
        self.whole_entry = "host" if seed % 2 else "device"
        self.retune = (int(rng.integers(1, n)), int(rng.integers(0, self.n_bands)), int(rng.integers(-32768, 32768))) if rng.random() < 0.5 else None
        if self.retune and self.retune[2] == self.steps[self.retune[1]]:
            self.retune = self.retune[:2] + (self.retune[2] ^ 1,)
        self.switch_at = int(rng.integers(1, n)) if rng.random() < 0.5 else None
        self.short_calls = sum(c * d < t - 1 for c in self.cuts)
        self.ident = (f"s{seed}-{R.FORMAT_IDS[self.fmt]}-D{d}-T{t}-c{self.chunk}x{self.threads}-b{self.n_bands}-{self.kind}-{first}"
                      + ("-retune" if self.retune else "") + ("-switch" if self.switch_at else ""))

    def _cuts(self, rng):
        """Outputs per call, adding up to self.outputs."""
        d, t, chunk, left = self.d, self.t, self.chunk, self.outputs
        groups = [[1], [chunk]]  # (a group stays together: the two short calls are consecutive)
        if t - 1 > 2 * d:
            short = min((t - 2) // d // 2, TILE // 4)  # (at D = 1 half the carry is more than the stream holds)
            assert short >= 1 and short * d < t - 1
            groups.append([short, short])
        left -= sum(sum(g) for g in groups)
        for c in (chunk - 1, chunk + 1):
            if 0 < c <= left:
                groups.append([c])
                left -= c
        while left > 0:
            c = min(left, int(rng.choice([1, 2, int(rng.integers(1, 2 * chunk + 2)), int(rng.integers(1, TILE + chunk + 2))])))
            groups.append([c])
            left -= c
        assert left == 0
        rng.shuffle(groups)
        return [c for g in groups for c in g]

    # -- the stream --------------------------------------------------------------------------------------------------------
    def taps(self):
        return np.random.default_rng(99_000 + self.seed).uniform(-1, 1, self.t).astype(np.float32)

    def raw(self):
        """The raw samples [outputs * D, 2] in the seed's format."""
        n, fmt = self.outputs * self.d, self.fmt
        rng = np.random.default_rng(111_000 + self.seed)
        if self.kind == "zeros":
            x = np.zeros((n, 2), R.RAW_DTYPE[fmt])
            if fmt == R.F32:
                x[rng.random((n, 2)) < 0.5] = -0.0
            return x
        x = R.random_raw(n, fmt, 222_000 + self.seed)
        if self.kind == "nonfinite":
            # a plant reaches ceil(T / D) outputs of every band; the seven sit a gap apart, T + 8 D samples where the stream
            # is long enough for that (each plant alone in front of some outputs) and closer where T / D is large, so that
            # all of them together reach at most 45 % of the outputs.  Each sits on a multiple of D, the sample that meets
            # tap 0: where T < D the others meet no tap at all
            gap = max(self.d, min(self.t + 8 * self.d, (45 * n // 100 - self.t) // (len(PLANTS) - 1)))
            at = int(rng.integers(0, n - gap * (len(PLANTS) - 1)))
            for i, p in enumerate(PLANTS):
                x[(at + i * gap) // self.d * self.d] = p
        elif self.kind == "full_scale":
            info = np.iinfo(R.RAW_DTYPE[fmt])
            for _ in range(4):
                a = int(rng.integers(0, n - 1))
                e = min(n, a + int(rng.integers(3, 2 * self.t + 8)))
                x[a:e] = rng.choice(np.array([info.min, info.max], R.RAW_DTYPE[fmt]), size=(e - a, 2))
        return x

    def pieces(self, raw):
        at = np.cumsum([0] + self.cuts) * self.d
        return [raw[a:e] for a, e in zip(at[:-1], at[1:])]

    # -- the reference -----------------------------------------------------------------------------------------------------
    def reference(self, cos, sin, raw=None):
        """(whole, cut): float32 [bands, outputs, 2] of the whole-stream call and of the calls along the cuts - the same array
        unless a retune makes the retuned band differ from its call on."""
        x = R.to_f32(self.raw() if raw is None else raw, self.fmt)
        with np.errstate(all="ignore"):
            whole = R.ddc_ref(x, self.d, self.taps(), self.steps, cos, sin, first_sample=self.first)
            if not self.retune:
                return whole, whole
            call, band, step = self.retune
            cut = whole.copy()
            cut[band] = self.reference_cut(cos, sin, x, bands=[band])[0]
        return whole, cut

    def reference_cut(self, cos, sin, x, bands=None, retune=True):
        """The reference run call by call along the cuts (of `bands` only, by default of all)."""
        bands = list(range(self.n_bands)) if bands is None else bands
        ref = R.DdcRef(self.d, self.taps(), [self.steps[b] for b in bands], cos, sin, first_sample=self.first)
        out = []
        with np.errstate(all="ignore"):
            for i, p in enumerate(self.pieces(x)):
                if retune and self.retune and i == self.retune[0] and self.retune[1] in bands:
                    ref.steps[bands.index(self.retune[1])] = self.retune[2]
                out.append(ref.process(p))
        return np.concatenate(out, axis=1)

    def same(self):
        """The name of the comparison in parity_tools: bit for bit, a NaN's sign and payload excepted where NaNs are made."""
        return "nan_equal_bits" if self.kind == "nonfinite" else "bits_equal"


def seeds(n=DEFAULT_SEEDS):
    return [Seed(s) for s in range(n)]
