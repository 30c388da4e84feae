"""The seeded generator of tests/test_fine_fuzz_gpu.py (pure NumPy: tests/test_fine_fuzz_coverage.py runs it without a GPU
and proves what the default seeds reach).

The fine converter's kernel (csrc/k_fine.hip) takes the down-converter's nine tile shapes (ddc_fuzz_gen.TABLE, shape) but
mixes its span with a loop of its own - the walk row += threads % D, col += threads / D, the carry and the stream of the
input the band points at.  The tables, the shape rule, the stream's length of 2 * TILE + chunk + 1 outputs and the cuts are
ddc_fuzz_gen's, imported and not restated.  A seed draws
  (D, T)             the first 18 seeds walk the nine shape classes twice, a class's first and last example geometry; later
                     seeds draw D in 1 .. 256 and T in 1 .. 4096;
  n_inputs           from INPUTS, lowered where the inputs' bytes would exceed INPUT_BYTES_CAP;
  n_bands            from ddc_fuzz_gen.BANDS under its cost cap;
  the input map      the bands dealt over `used` inputs, fewer than the bands where there are two or more, so several bands
                     read one input; with two or more inputs one, `spare`, is read by nobody;
  steps              per band from ddc_fuzz_gen.STEPS or random;
  the first sample   ddc_fuzz_gen.FIRSTS: 0, a multiple of D, or one that puts 2^31 or 2^32 inside the run;
  cuts               ddc_fuzz_gen.Seed._cuts: a call of D samples, one of exactly `chunk` outputs, chunk - 1 and chunk + 1,
                     two consecutive calls shorter than T - 1 samples, the rest drawn;
  events             in front of calls of the cut run: "move" - sdr_fine_set_input takes a band to the spare input, whose
                     carry nobody has used so far, and a later call takes it back; "retune" - sdr_fine_set_nco_step;
                     "switch" - sdr_fine_set_stream with a second stream;
  gaps               between the inputs and behind a band's outputs (fine_run.run_gpu), 0 among them, for the whole run and
                     for the cut run;
  the value kind     "plain"      uniform in [-1, 1)
                     "zeros"      all-zero inputs with drawn signs: every output word is +0
                     "nonfinite"  the seven ddc_fuzz_gen.PLANTS in single samples of every input, placed by its rule: at
                                  least half of the outputs stay finite (compared with nan_equal_bits)
                     "subnormal"  inputs and taps scaled so that every output is subnormal and more than 90 % are nonzero.
Among the table's seeds the zeros go to the classes of one output per lane only, for ddc_fuzz_gen's reason: an all-zero
result cannot tell a lane's two outputs apart.  A plain helper module, not a test file."""
import numpy as np

import ddc_fuzz_gen as D
import fine_ref as F
from ddc_fuzz_gen import BANDS, CLASSES, COST_CAP, FIRSTS, MAX_D, MAX_T, PLANTS, STEPS, TABLE, TILE, shape  # noqa: F401

DEFAULT_SEEDS = 2 * len(TABLE)
INPUTS = (1, 2, 3, 17, 256)
INPUT_BYTES_CAP = 64 << 20
GAPS = (0, 4, 8, 12)
KINDS = ("plain", "zeros", "nonfinite", "subnormal")
EVENTS = ("move", "retune", "switch")


class Seed:
    """Everything one seed draws; streams() makes the inputs, reference(cos, sin) what the fine converter must deliver."""

    def __init__(self, seed):
        self.seed = seed
        rng = np.random.default_rng(55_000 + seed)
        table_class = seed % len(TABLE) if seed < DEFAULT_SEEDS else None
        if table_class is not None:
            examples = TABLE[table_class][1]
            self.d, self.t = examples[0] if seed < len(TABLE) else examples[-1]
            bands, first, n_inputs = BANDS[(seed + 1) % len(BANDS)], FIRSTS[seed % len(FIRSTS)], INPUTS[(seed + 4) % len(INPUTS)]
        else:
            self.d = int(rng.choice([int(rng.integers(1, 9)), int(rng.integers(1, MAX_D + 1)), int(rng.integers(30, MAX_D + 1))]))
            self.t = int(rng.choice([int(rng.integers(1, 65)), int(rng.integers(1, MAX_T + 1)), int(rng.integers(MAX_T - 200, MAX_T + 1))]))
            bands, first, n_inputs = int(rng.choice(BANDS)), str(rng.choice(FIRSTS)), int(rng.choice(INPUTS))
        d, t = self.d, self.t
        self.chunk, self.threads, self.width, self.lds_bytes = shape(d, t)
        self.cls = (self.chunk, self.threads)
        assert table_class is None or self.cls == CLASSES[table_class], (seed, self.cls)
        self.outputs = m = 2 * TILE + self.chunk + 1
        self.n = m * d
        self.n_inputs = max(i for i in INPUTS if i <= n_inputs and (i == 1 or i * self.n * 8 <= INPUT_BYTES_CAP))
        self.n_bands = max(b for b in BANDS if b <= bands and (b == 1 or b * t * m <= COST_CAP))
        self.cost = self.n_bands * t * m
        self.steps = [int(STEPS[i]) if i < len(STEPS) else int(rng.integers(-32768, 32768)) for i in rng.integers(0, len(STEPS) + 1, self.n_bands)]
        # the map: `spare` is read by nobody; the bands share the `used` inputs
        order = [int(i) for i in rng.permutation(self.n_inputs)]
        self.spare = order.pop() if self.n_inputs >= 2 else None
        n_used = max(1, min(len(order), self.n_bands - 1 if self.n_bands > 1 else 1, int(rng.integers(2, 9))))
        self.used = sorted(order[:n_used])
        if self.n_inputs == max(INPUTS) and self.spare != self.n_inputs - 1:
            self.used[-1] = self.n_inputs - 1  # (the limit: the last of 256 inputs is read)
        self.inputs = [self.used[b % n_used] for b in range(n_used)] + [int(rng.choice(self.used)) for _ in range(self.n_bands - n_used)]
        self.inputs = [self.inputs[i] for i in rng.permutation(len(self.inputs))][:self.n_bands]
        self.kind = self._kind(rng, table_class)
        self.first_kind = first
        if first == "zero":
            self.first = 0
        elif first == "multiple":
            self.first = int(rng.integers(1, 1 << 20)) * d
        else:  # the edge lies inside the run
            edge = 2 ** 31 if first == "2^31" else 2 ** 32
            self.first = (edge - int(rng.integers(d, (m - 1) * d + 1))) // d * d
            assert self.first < edge < self.first + m * d
        self.cuts = D.Seed._cuts(self, rng)  # (the down-converter fuzz's rules, on this seed's D, T, chunk and outputs)
        n = len(self.cuts)
        self.short_calls = sum(c * d < t - 1 for c in self.cuts)
        # the events: {call: [(setter, band, value)]} and the call of the stream switch
        pick = (lambda e: (seed + EVENTS.index(e)) % 4 != 0) if table_class is not None else (lambda e: rng.random() < 0.6)
        self.changes, self.events = {}, set()
        if pick("move") and self.spare is not None and n >= 3:
            a = int(rng.integers(1, n - 1))
            z = int(rng.integers(a + 1, n))
            band = int(rng.integers(0, self.n_bands))
            self.changes.setdefault(a, []).append(("set_input", band, self.spare))
            self.changes.setdefault(z, []).append(("set_input", band, self.inputs[band]))
            self.events.add("move")
        if pick("retune"):
            band = int(rng.integers(0, self.n_bands))
            step = int(rng.integers(-32768, 32768))
            self.changes.setdefault(int(rng.integers(1, n)), []).append(("set_nco_step", band, step ^ 1 if step == self.steps[band] else step))
            self.events.add("retune")
        self.switch_at = int(rng.integers(1, n)) if pick("switch") else None
        if self.switch_at is not None:
            self.events.add("switch")
        self.gaps = tuple(int(g) for g in rng.choice(GAPS, 4))  # (in, out) of the whole run, (in, out) of the cut run
        self.ident = (f"s{seed}-D{d}-T{t}-c{self.chunk}x{self.threads}-i{self.n_inputs}-b{self.n_bands}-{self.kind}-{first}"
                      + "".join("-" + e for e in EVENTS if e in self.events))

    def _kind(self, rng, table_class):
        if table_class is None:
            kind = str(rng.choice(KINDS))
            # (ddc_fuzz_gen's rule: where seven plants cannot leave half of the outputs finite, the seed is a plain one)
            return "plain" if kind == "nonfinite" and self.t + len(PLANTS) * self.d > 45 * self.n // 100 else kind
        pool = ("plain", "nonfinite", "subnormal") if self.chunk > self.threads else ("zeros", "nonfinite", "subnormal", "plain")
        return pool[(table_class + 2 * (self.seed // len(TABLE))) % len(pool)]

    # -- the streams -------------------------------------------------------------------------------------------------------
    def taps(self):
        taps = np.random.default_rng(66_000 + self.seed).uniform(-1, 1, self.t)
        return (taps * (1e-10 if self.kind == "subnormal" else 1.0)).astype(np.float32)

    def streams(self):
        """float32 [n_inputs, outputs * D, 2]"""
        n, d, t = self.n, self.d, self.t
        rng = np.random.default_rng(111_000 + self.seed)
        if self.kind == "zeros":
            x = np.zeros((self.n_inputs, n, 2), np.float32)
            x[rng.random(x.shape) < 0.5] = -0.0
            return x
        x = rng.random((self.n_inputs, n, 2), dtype=np.float32) * np.float32(2.0) - np.float32(1.0)
        if self.kind == "subnormal":
            # tap * sample is about 1e-40 at the most; the sum of T of them stays below the smallest normal number, 1.2e-38
            x = (x * np.float32(1e-30 if t <= 1024 else 2.5e-31)).astype(np.float32)
        elif self.kind == "nonfinite":
            # ddc_fuzz_gen.Seed.raw's placing: a gap apart, each on a multiple of D, all seven reaching at most 45 % of the outputs
            gap = max(d, min(t + 8 * d, (45 * n // 100 - t) // (len(PLANTS) - 1)))
            at = int(rng.integers(0, n - gap * (len(PLANTS) - 1)))
            for i, p in enumerate(PLANTS):
                x[:, (at + i * gap) // d * d] = p
        return x

    def pieces(self, x):
        at = np.cumsum([0] + self.cuts) * self.d
        return [x[:, a:e] for a, e in zip(at[:-1], at[1:])]

    def between(self, obj, i):
        """In front of call i of the cut run: on the library's object or on the reference's."""
        for name, band, value in self.changes.get(i, ()):
            getattr(obj, name)(band, value)

    # -- the reference -----------------------------------------------------------------------------------------------------
    def reference(self, cos, sin, x=None):
        """(whole, cut): float32 [bands, outputs, 2] of the whole-stream call and of the calls along the cuts with their
        events.  A band's outputs of one call use the step and the input current in that call for all their taps, and every
        input's carry is the raw stream's: the cut run's band is, call by call, the whole-stream band of the (step, input)
        current there.  (tests/test_fine_fuzz_coverage.py holds this to fine_ref.FineRef run call by call.)"""
        x = self.streams() if x is None else x
        state = list(zip(self.steps, self.inputs))
        per_call = []
        for i in range(len(self.cuts)):
            for name, band, value in self.changes.get(i, ()):
                state[band] = (value, state[band][1]) if name == "set_nco_step" else (state[band][0], value)
            per_call.append(list(state))
        pairs = sorted(set(zip(self.steps, self.inputs)) | {p for c in per_call for p in c})
        with np.errstate(all="ignore"):
            ref = F.fine_ref(x, self.d, self.taps(), [p[0] for p in pairs], cos, sin, inputs=[p[1] for p in pairs], first_sample=self.first)
        whole = np.stack([ref[pairs.index(p)] for p in zip(self.steps, self.inputs)])
        cut = np.empty_like(whole)
        at = np.cumsum([0] + self.cuts)
        for i, c in enumerate(per_call):
            for b, p in enumerate(c):
                cut[b, at[i]:at[i + 1]] = ref[pairs.index(p), at[i]:at[i + 1]]
        return whole, cut

    def reference_cut(self, cos, sin, x, events=True):
        """fine_ref.FineRef call by call along the cuts."""
        ref = F.FineRef(self.n_inputs, self.d, self.taps(), self.steps, cos, sin, inputs=self.inputs, first_sample=self.first)
        out = []
        with np.errstate(all="ignore"):
            for i, p in enumerate(self.pieces(x)):
                if events:
                    self.between(ref, i)
                out.append(ref.process(p))
        return np.concatenate(out, axis=1)

    def same(self):
        """The name of the comparison in parity_tools: bit for bit, a NaN's sign and payload excepted where NaNs are made."""
        return "nan_equal_bits" if self.kind == "nonfinite" else "bits_equal"


def seeds(n=DEFAULT_SEEDS):
    return [Seed(s) for s in range(n)]
