"""Inputs that put peak runs where the peak scan's subtle code sits (k_peaks.hip): at word ends (64 bins), at the
refinement's span ends (4096 bins, 16384 in the wide shape), at bin 0 and N - 1, over more than a word, and more runs than
the bank's max_peaks holds; and a keying that makes more edges than a batch stores (k_listen.hip).  Pure numpy, a plain
module like fuzz_paths_gen.py: tests/test_peak_shape_host.py confirms every case on the oracle alone,
tests/test_peak_shape_gpu.py runs the same cases on the bank.

Two frame makers:
  shaped        noise of synth.NOISE_SIGMA and runs of bins raised 35 dB over it, one bin of each run - the designated
                maximum - another 6 dB higher, a fresh random phase per bin and frame
  shifted_tied  fuzz_paths_gen.tied_peak_frames with the spectrum moved by `shift` bins (the four non-zero samples times
                powers of i: exact): exactly tied pairs 4k + 3, 4k + 4 for shift 3 - across every word and span end -
                and single-bin runs at 0 and N - 1
"""
import functools

import numpy as np

import fuzz_paths_gen
from sdrainer_amd import synth

RATES = {512: 48_000, 8192: 2_000_000, 16384: 2_000_000, 32768: 2_000_000}
RAISE_DB = 35.0
WORD = 64
SHIFT = 3
TIED_THRESHOLD = fuzz_paths_gen.TIED_PEAK_THRESHOLD
EDGE_CAP = 8192  # edges a batch stores per listener: min(max_batch_frames, 8192) (capi_bank.hip)


def noise_windows(n, edge):
    """The first nine of the reference's noise-floor windows, [from, to) in spectrum bins (the tenth is not evaluated in
    every geometry: it is not counted on)."""
    w = (n - 2 * edge) // 10
    return [(edge + k * w, edge + (k + 1) * w) for k in range(9)]


def shaped(n, frames, runs, seed):
    """float32 [frames, 2N].  runs: (from, to, max_bin) or (from, to, max_bin, frames_on) - a run with frames_on is raised
    in the first frames_on frames only."""
    runs = [tuple(r) + (frames,) * (4 - len(r)) for r in runs]
    taken = set()
    for a, e, m, _ in runs:
        assert 0 <= a <= m <= e < n, (a, e, m)
        assert not taken & set(range(a - 1, e + 2)), f"run {a} - {e} touches another"
        taken |= set(range(a, e + 1))
    assert any(not taken & set(range(lo, hi)) for lo, hi in noise_windows(n, synth.default_edge_width(n))), \
        "every noise-floor window holds a raised bin: the minimum window mean is no longer noise"
    sigma = synth.NOISE_SIGMA
    unit = sigma * np.sqrt(2.0 * n) * 10.0 ** (RAISE_DB / 20.0)
    bins = np.array([b for a, e, _, _ in runs for b in range(a, e + 1)], np.int64)
    mag = np.array([unit * (2.0 if b == m else 1.0) for a, e, m, _ in runs for b in range(a, e + 1)])
    on = np.array([k for a, e, _, k in runs for b in range(a, e + 1)], np.int64)
    fft_bins = (bins + n // 2) % n  # spectrum index -> FFT index, as synth.make_band
    rng = np.random.default_rng(seed)
    iq = np.empty((frames, 2 * n), np.float32)
    chunk = max(1, (1 << 21) // n)
    for f0 in range(0, frames, chunk):
        f1 = min(frames, f0 + chunk)
        spec = np.zeros((f1 - f0, n), np.complex128)
        phase = rng.random((f1 - f0, len(bins))) * (2.0 * np.pi)
        live = (np.arange(f0, f1)[:, None] < on[None, :])
        spec[:, fft_bins] = mag[None, :] * live * np.exp(1j * phase)
        x = np.fft.ifft(spec, axis=1)
        x += sigma * (rng.standard_normal((f1 - f0, n)) + 1j * rng.standard_normal((f1 - f0, n)))
        iq[f0:f1, 0::2] = x.real
        iq[f0:f1, 1::2] = x.imag
    return iq


def shifted_tied(rng, n, frames, shift):
    """fuzz_paths_gen.tied_peak_frames with sample m N / 4 multiplied by i^((shift m) % 4): the spectrum moves by `shift`
    bins, exactly (a multiplication by +-1 or +-i), and the ties stay exact."""
    out = fuzz_paths_gen.tied_peak_frames(rng, n, frames)
    for m in range(4):
        at = 2 * (m * n // 4)
        z = (out[:, at] + 1j * out[:, at + 1]) * (1j ** ((shift * m) % 4))
        out[:, at], out[:, at + 1] = z.real, z.imag
    return out


def tied_runs(n, shift=SHIFT):
    """The runs of a shifted_tied cumulation: the pairs 4k + shift, 4k + shift + 1 cut at the row's ends, first maximum."""
    assert shift == 3
    return [(0, 0, 0)] + [(b, b + 1, b) for b in range(3, n - 4, 4)] + [(n - 1, n - 1, n - 1)]


def spans(n):
    """Where a refinement span ends inside the row: 4096 bins in the narrow shape (its multiples at N = 16384, the largest
    row held in LDS), 16384 in the wide one."""
    return {512: [], 8192: [4096], 16384: [4096, 8192, 12288], 32768: [4096, 16384]}[n]


def geometry_runs(n, case):
    """The runs of the named geometry cases (the table of tests/test_peak_shape_gpu.py's docstring)."""
    w, S = WORD, spans(n)
    if case == "a":  # a run at either end of the row, across a word end (maximum behind it), two whole words
        return [(0, 2, 0), (w - 2, w + 1, w), (2 * w - 1, 2 * w - 1, 2 * w - 1), (4 * w, 4 * w, 4 * w), (310, 450, 400),
                (n - 7, n - 1, n - 1)] + [(s - 2, s + 1, s - 1) for s in S]
    if case == "b":  # single bins at either end of the row and either side of a word end, maxima in front of the ends.  The
        # run with its maximum on a word's last bit lies across the SECOND word's end, (2w - 2, 2w + 1: 2w - 1): the single
        # bins 63 and 65 occupy the first word's end, and `flags[w - 1] >> 63` is the same code at every word
        return [(0, 0, 0), (63, 63, 63), (65, 65, 65), (2 * w - 2, 2 * w + 1, 2 * w - 1), (3 * w - 1, 3 * w - 1, 3 * w - 1),
                (5 * w, 5 * w, 5 * w), (n - 1, n - 1, n - 1)] + [(s - 2, s + 1, s) for s in S]
    if case == "c":  # one run from mid-word through to N - 1 over three words and more; the last bin of a span
        return [(s - 1, s - 1, s - 1) for s in S] + [(n - 230, n - 1, n - 230)]
    if case == "d":  # the first bin of a span; runs at the row's ends with the maximum at the inner end
        assert S
        return [(0, 2, 2)] + [(s, s, s) for s in S] + [(n - 7, n - 1, n - 7)]
    raise KeyError(case)


# the runs of the capacity case: nine in the first cumulation, two from then on
CAPACITY_RUNS = [(0, 1, 1), (40, 40, 40, 100), (63, 64, 63, 100), (100, 104, 102, 100), (127, 127, 127, 100), (129, 129, 129),
                 (200, 260, 230, 100), (300, 300, 300, 100), (505, 511, 511, 100)]
# the listener row (N = 16384): listeners, and the runs they sit on
LISTENER_BINS = [0, 16383, 4095, 4096, 4097, 8191, 12288, 10000]
LISTENER_RUNS = [(0, 2, 0), (4093, 4099, 4096), (8190, 8192, 8191), (10000, 10005, 10003), (12288, 12288, 12288), (16377, 16383, 16383)]


class Band:
    """One band's input: kind "shaped" (runs) or "tied"; expected(c) = the (from, to, signal_bin) of cumulation c."""

    def __init__(self, n, frames, kind, runs=None, seed=0, threshold=15.0):
        self.n, self.frames, self.kind, self.seed = n, frames, kind, seed
        self.runs = tuple(tuple(r) for r in (runs or ()))
        self.threshold = TIED_THRESHOLD if kind == "tied" else threshold

    @property
    def key(self):
        return (self.n, self.frames, self.kind, self.runs, self.seed)

    def iq(self):
        return _frames(self.key)

    def expected(self, c):
        if self.kind == "tied":
            return tied_runs(self.n)
        return sorted(r[:3] for r in self.runs if len(r) < 4 or r[3] >= 100 * (c + 1))


@functools.lru_cache(maxsize=4)
def _frames(key):
    n, frames, kind, runs, seed = key
    iq = shifted_tied(np.random.default_rng(seed), n, frames, SHIFT) if kind == "tied" else shaped(n, frames, runs, seed)
    iq.setflags(write=False)
    return iq


class Row:
    """One row of tests/test_peak_shape_gpu.py: the bands, the batch cuts, the input path, the bank's max_peaks and the
    listeners of every band."""

    def __init__(self, id, bands, batches, path="device", max_peaks=None, listeners=None):
        self.id, self.bands, self.batches, self.path = id, bands, list(batches), path
        self.n, self.frames = bands[0].n, sum(batches)
        assert all(b.n == self.n and b.frames == self.frames for b in bands)
        self.max_peaks = max_peaks if max_peaks is not None else max(64, self.n // 4 + 16)
        self.listeners = listeners if listeners is not None else [[] for _ in bands]
        self.cumulations = self.frames // 100

    def counts(self, band=0):
        return [len(self.bands[band].expected(c)) for c in range(self.cumulations)]


CUTS = [99, 1, 98, 2, 97, 3, 100]  # cumulations that begin with a first slot of 1, 2 and 3 frames; one batch = one cumulation
UNEVEN = {512: [37, 163, 30], 8192: [131, 99], 16384: [61, 150, 19], 32768: [203, 97]}


def _shaped(n, case, frames, seed=None):
    return Band(n, frames, "shaped", geometry_runs(n, case), seed=1000 + n // 64 + ord(case) if seed is None else seed)


def _geometry():
    rows = []
    for n in (512, 8192, 16384, 32768):
        for case in "abcd" if spans(n) else "abc":
            rows.append(Row(f"n{n}-{case}", [_shaped(n, case, sum(UNEVEN[n]))], UNEVEN[n]))
    for n in (512, 8192):
        rows.append(Row(f"n{n}-tied", [Band(n, sum(UNEVEN[n]), "tied", seed=77 + n)], UNEVEN[n]))
        rows.append(Row(f"n{n}-a-cuts", [_shaped(n, "a", sum(CUTS))], CUTS))
    rows.append(Row("n512-tied-cuts", [Band(512, sum(CUTS), "tied", seed=78)], CUTS))
    rows.append(Row("n512-b-graph", [_shaped(512, "b", 240)], [40] * fuzz_paths_gen.GRAPH_BATCHES, path="graph"))
    rows.append(Row("n512-a-staged", [_shaped(512, "a", sum(UNEVEN[512]))], UNEVEN[512], path="staged"))
    rows.append(Row("n8192-two-bands", [_shaped(8192, "a", 230), _shaped(8192, "b", 230)], UNEVEN[8192]))
    return rows


GEOMETRY = _geometry()
LISTENERS = [Row("n16384-listeners", [Band(16384, 230, "shaped", LISTENER_RUNS, seed=1601)], UNEVEN[16384], listeners=[LISTENER_BINS])]
CAPACITY = ([Row(f"n512-tied-max{m}", [Band(512, 230, "tied", seed=589)], UNEVEN[512], max_peaks=m) for m in (1, 64, 129)]
            + [Row("n512-nine-max4", [Band(512, 330, "shaped", CAPACITY_RUNS, seed=1512)], [130, 200], max_peaks=4),
               Row("n512-nine-max4-one-batch", [Band(512, 330, "shaped", CAPACITY_RUNS, seed=1512)], [330], max_peaks=4)])
EXACT_FIT = "n512-tied-max129"
GROUP = Row("n512-group-max4", [Band(512, 330, "shaped", CAPACITY_RUNS, seed=1512), Band(512, 330, "tied", seed=590)], [330], max_peaks=4)
ROWS = GEOMETRY + LISTENERS + CAPACITY + [GROUP]

# every test of tests/test_peak_shape_gpu.py by node id, and the N = 16384 rows among them (tests/test_forced_paths.py runs
# them under the forced switches and counts what passed)
MODULE = "tests/test_peak_shape_gpu.py"
NODE_IDS = ([f"{MODULE}::test_peak_geometry[{r.id}]" for r in GEOMETRY + LISTENERS] + [f"{MODULE}::test_peak_capacity[{r.id}]" for r in CAPACITY]
            + [f"{MODULE}::{t}" for t in ("test_peak_capacity_through_a_group", "test_edge_capacity_read", "test_edge_capacity_polled")])
NODE_IDS_16384 = [x for x in NODE_IDS if "[n16384-" in x]

# -- the edge row ----------------------------------------------------------------------------------------------------------
EDGE_N, EDGE_RATE, EDGE_FRAMES, EDGE_TAIL = 512, 48_000, 8400, 2000


def edge_stream():
    """(float32 [8400 + 2000, 2N], the listener's bin): a carrier on in even frames only - an edge per frame, more than a
    batch stores - and behind it synth.make_band's keyed carrier on the same bin."""
    n = EDGE_N
    tail, bins, _ = synth.make_band(EDGE_TAIL, EDGE_RATE, n, 1, seed=8400)
    b = int(bins[0])
    tone = synth.TONE_AMPLITUDE * np.exp(2j * np.pi * ((b + n // 2) % n) * np.arange(n) / n)
    rng = np.random.default_rng(8401)
    on = (np.arange(EDGE_FRAMES) % 2 == 0).astype(np.float64)
    x = on[:, None] * tone[None, :] + synth.NOISE_SIGMA * (rng.standard_normal((EDGE_FRAMES, n)) + 1j * rng.standard_normal((EDGE_FRAMES, n)))
    head = np.empty((EDGE_FRAMES, 2 * n), np.float32)
    head[:, 0::2], head[:, 1::2] = x.real, x.imag
    return np.concatenate([head, tail]), b
