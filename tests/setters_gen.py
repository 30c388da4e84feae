"""The controls of a running bank - sdr_set_signal_debounce, sdr_set_edge_width, sdr_set_peak_threshold, sdr_set_find_peaks -
turned between the batches of a stream: the table of cases that tests/test_setters_gpu.py runs against the oracle and
tests/test_setters_reach.py reads on the CPU, so that the reach test asserts on the very inputs the GPU tests run.  A plain
helper module, not a test file: numpy and the CPU oracle only, nothing of the GPU.

Every case is a parity_case.Case over keyed carriers of tests/keying_gen.py (kinds whose raw states glitch), its steps
holding ("set", name, band, value) between the batches."""
import functools

import numpy as np

import iq8_tools
from keying_gen import key_matrix, keyed_band
from parity_tools import random_window, sc16_to_float32
from sdrainer_amd import synth

N, RATE = 512, 48_000
EDGE = synth.default_edge_width(N)
GRAPH_BATCHES = 6  # sdr_graph_batches(): the graph row's steps are cut for it (the test asserts the bank agrees)


def nine_window_edge(n):
    """An edge width with N - 2 edge a multiple of ten: the reference evaluates nine windows (fuzz_paths_gen.tied_window)."""
    import fuzz_paths_gen

    e = fuzz_paths_gen.tied_window(n)[0]
    assert (n - 2 * e) % 10 == 0
    return e


def one_bin_edge(n):
    """(N - 10) / 2: ten bins left, a window of one bin."""
    return (n - 10) // 2


def edge_sequence(n):
    """default -> 1 -> nine windows -> windows of one bin -> 0 -> default."""
    return [1, nine_window_edge(n), one_bin_edge(n), 0, synth.default_edge_width(n)]


def band_input(n, frames, kinds, seed, path="device", hop=None, dits=None, amplitude=synth.TONE_AMPLITUDE):
    """(float32, what the path sends or None, the carriers' bins) of `frames` frames of carriers keyed by `kinds`: dense frames
    [F, 2N], or with a hop the stream [samples, 2].  For sc16 and 8-bit paths the float32 values are the quantised ones'."""
    iq8 = path in ("device_cs8", "device_cu8")
    rows = frames - 1 + n // hop if hop else frames
    keys = key_matrix(rows, kinds, seed, dits)
    f32, q, bins = keyed_band(n, RATE, keys, seed + 50, amplitude=amplitude, hop=hop, sigma=iq8_tools.SIGMA if iq8 else synth.NOISE_SIGMA)
    if path in ("device_sc16", "staged_sc16", "kiwi", "graph_sc16"):
        q = np.rint(f32.astype(np.float64) * (30000.0 / float(np.abs(f32).max()))).astype(np.int16)
        f32 = sc16_to_float32(q)
    elif iq8:
        fmt = iq8_tools.CS8 if path == "device_cs8" else iq8_tools.CU8
        q = iq8_tools.quantise(f32, fmt)
        f32 = iq8_tools.to_f32(q, fmt)
    return np.ascontiguousarray(f32), q, bins


def _case(n, bands, init_bins, steps, seed, **kw):
    from parity_case import Case

    return Case(n, len(bands), None, 0, steps, seed, rate=RATE, bands=bands, init_bins=init_bins, **kw)


# -- (1) the debounce sequence ---------------------------------------------------------------------------------------------
# One band, twelve carriers, 70 listeners: the carriers, 46 bins beside and between them, the carriers once more - slots 58 - 69
# are keyed, and k_set_debounce's second workgroup (slots 64 - 69) holds jitter, fast, noise and dahs carriers.  A bank created
# at debounce 1; 1 -> 3 -> 1 -> 5 -> 70 -> 2 -> 0 -> 3 between the batches, one of them a single frame.  DEB_FRESH is attached
# behind the 5 and gets a slot of its own: it runs at the bank's debounce 1 beside listener 1, on the same bin at 5 and then,
# when the 70 reaches both, at 70.  Listener DEB_GONE is detached in front of the 70, which must pass its slot by; DEB_REUSE is
# attached behind the 2 into that slot (an attach takes the lowest free one) and runs at 1 again.
DEB_SEED = 8100
DEB_KINDS = ("noise", "jitter", "clean", "sparse", "long", "noise", "jitter", "fast", "noise", "jitter", "dahs", "noise")
DEB_VALUES = (3, 1, 5, 70, 2, 0, 3)
DEB_BATCHES = (300, 200, 1, 150, 250, 200, 100, 200)
DEB_LISTENERS, DEB_GONE, DEB_FRESH, DEB_REUSE = 70, 3, 70, 71  # (the oracle's numbering: 70 and 71 are the late ones)


@functools.lru_cache(maxsize=None)
def deb_band():
    return band_input(N, sum(DEB_BATCHES), DEB_KINDS, DEB_SEED)


def deb_bins():
    from parity_case import _extra_bins

    bins = deb_band()[2]
    return bins + _extra_bins(N, bins, DEB_LISTENERS - 2 * len(bins), DEB_SEED) + bins


def deb_steps():
    bins = deb_band()[2]
    steps = []
    for i, frames in enumerate(DEB_BATCHES):
        steps.append(("batch", frames))
        if i == len(DEB_VALUES):
            break
        if DEB_VALUES[i] == 70:
            steps.append(("detach", 0, DEB_GONE))
        steps.append(("set", "signal_debounce", 0, DEB_VALUES[i]))
        if DEB_VALUES[i] == 5:
            steps.append(("attach", 0, bins[1]))
        if DEB_VALUES[i] == 2:
            steps.append(("attach", 0, bins[0]))
    return steps


def case_debounce():
    return _case(N, [deb_band()], [deb_bins()], deb_steps(), DEB_SEED, debounce=1, path="device")


# -- (2) per band ----------------------------------------------------------------------------------------------------------
# Three bands; the debounce and the peak threshold of band 1, then of band 2; band 0 is never touched.  Bands -1 and 3 are
# refused and change nothing.
BAND_SEED = 8200
BAND_KINDS = ("noise", "jitter", "clean", "noise", "jitter", "fast")
BAND_BATCHES = (200, 150, 150, 100)


@functools.lru_cache(maxsize=None)
def band_bands():
    return [band_input(N, sum(BAND_BATCHES), BAND_KINDS, BAND_SEED + b) for b in range(3)]


def case_bands():
    from parity_tools import listener_bins

    bands = band_bands()
    steps = [("batch", BAND_BATCHES[0]), ("set", "signal_debounce", 1, 4), ("set", "peak_threshold", 1, 9.0),
             ("set", "signal_debounce", 3, ("bad", 5)), ("set", "peak_threshold", 3, ("bad", 5.0)),
             ("batch", BAND_BATCHES[1]), ("set", "signal_debounce", 2, 3), ("set", "peak_threshold", 2, 21.5),
             ("set", "signal_debounce", -1, ("bad", 7)), ("set", "peak_threshold", -1, ("bad", 7.0)),
             ("batch", BAND_BATCHES[2]), ("set", "signal_debounce", 1, 2), ("batch", BAND_BATCHES[3])]
    return _case(N, bands, [listener_bins(N, b[2], 9) for b in bands], steps, BAND_SEED, debounce=1, path="device", trace=True)


# -- (3) the edge-width sequence -------------------------------------------------------------------------------------------
# default -> 1 -> nine windows -> one-bin windows -> 0 -> default.  The first setter falls at frame 130, in mid-cumulation; the
# batch behind the second completes the cumulations of frames 299 and 399.  Refused widths (-1, one that leaves 8 bins) in
# front of the last batch.
EDGE_SEED = 8300
EDGE_KINDS = ("clean", "jitter", "noise", "long", "clean", "fast", "jitter", "dahs")
EDGE_BATCHES = (130, 70, 230, 120, 90, 160)


@functools.lru_cache(maxsize=None)
def edge_band():
    return band_input(N, sum(EDGE_BATCHES), EDGE_KINDS, EDGE_SEED)


def edge_steps(n, batches):
    steps = []
    for frames, e in zip(batches, edge_sequence(n) + [None]):
        steps.append(("batch", frames))
        if e is not None:
            steps.append(("set", "edge_width", None, e))
    steps[-1:-1] = [("set", "edge_width", None, ("bad", -1)), ("set", "edge_width", None, ("bad", (n - 8) // 2))]
    return steps


def case_edge():
    from parity_tools import listener_bins

    band = edge_band()
    return _case(N, [band], [listener_bins(N, band[2], 12)], edge_steps(N, EDGE_BATCHES), EDGE_SEED, path="device", trace=True)


# -- (4) the peak-threshold sequence ---------------------------------------------------------------------------------------
# Two bands that start at 15 and 12 dB.  Carriers from 64 dB above the noise down to a few: what a threshold between 0 and
# 21.5 dB admits changes with it.  Every setter falls in mid-cumulation; the peak search is off for the cumulation of frame
# 399 and on again behind it; at the end +Inf on both bands.
PEAK_SEED = 8400
PEAK_KINDS = ("clean", "jitter", "long", "clean", "fast", "jitter", "dahs", "clean", "noise", "long")
PEAK_AMPLITUDE = tuple(float(x) for x in np.geomspace(0.1, 4e-4, len(PEAK_KINDS)))
PEAK_START = (15.0, 12.0)
PEAK_BATCHES = (150, 100, 100, 100, 120, 100, 130)
PEAK_STEPS = [("batch", 150), ("set", "peak_threshold", 0, 9.0), ("batch", 100), ("set", "peak_threshold", 1, 21.5), ("batch", 100),
              ("set", "find_peaks", None, False), ("batch", 100), ("set", "find_peaks", None, True), ("set", "peak_threshold", 0, 0.0),
              ("batch", 120), ("set", "peak_threshold", 1, -3.0), ("set", "peak_threshold", 0, float("inf")), ("batch", 100),
              ("set", "peak_threshold", 1, float("inf")), ("batch", 130)]


@functools.lru_cache(maxsize=None)
def peak_bands():
    return [band_input(N, sum(PEAK_BATCHES), PEAK_KINDS, PEAK_SEED + b, amplitude=np.array(PEAK_AMPLITUDE)) for b in range(2)]


def case_peaks():
    bands = peak_bands()
    return _case(N, bands, [b[2] for b in bands], list(PEAK_STEPS), PEAK_SEED, threshold=list(PEAK_START), path="device", trace=True)


# -- (5) paths -------------------------------------------------------------------------------------------------------------
# Both sequences, shortened, in one stream: every cut takes a debounce and an edge-width setter.  (name, N, path, hop, windowed)
PATH_SEED = 8500
PATH_KINDS = ("noise", "jitter", "clean", "noise", "jitter", "fast")
PATH_BATCHES = (230, 170, 1, 160, 139)
PATH_DEBOUNCE = (3, 0, 5, 2)
PATH_ROWS = (("staged", 512, "staged", None, False), ("device_sc16", 512, "device_sc16", None, False),
             ("device_cs8", 512, "device_cs8", None, False), ("hop", 1024, "device", 256, False),
             ("windowed", 512, "device", None, True))
PATH_HOP_DITS = (5, 10)  # a frame spans four hops: a carrier is up while any of them is, so gaps lose three ticks


def path_edges(n):
    return [1, nine_window_edge(n), one_bin_edge(n), synth.default_edge_width(n)]


def case_path(row):
    from parity_tools import listener_bins

    name, n, path, hop, win = next(r for r in PATH_ROWS if r[0] == row)
    band = band_input(n, sum(PATH_BATCHES), PATH_KINDS, PATH_SEED + n, path, hop, PATH_HOP_DITS if hop else None)
    steps = []
    for i, frames in enumerate(PATH_BATCHES):
        steps.append(("batch", frames))
        if i < len(PATH_DEBOUNCE):
            steps += [("set", "signal_debounce", 0, PATH_DEBOUNCE[i]), ("set", "edge_width", None, path_edges(n)[i])]
    windows = [random_window(n, PATH_SEED)] * len(PATH_BATCHES) if win else None
    return _case(n, [band], [listener_bins(n, band[2], 10)], steps, PATH_SEED, debounce=1, path=path, hop=hop, windows=windows, trace=True)


# -- (6) graph -------------------------------------------------------------------------------------------------------------
# Four replays of six batches of 60 frames.  Behind the first: debounce 3 and a peak threshold of 9 dB - the next replay takes
# them with the capture in place; behind the second: edge width 1 - the replay is refused, release, capture; behind the third:
# edge width 1 again, debounce 0 - no new capture.
GRAPH_SEED, GRAPH_PER = 8600, 60
GRAPH_KINDS = PATH_KINDS


def case_graph(path="graph"):
    from parity_tools import listener_bins

    replay = [("batch", GRAPH_PER)] * GRAPH_BATCHES
    band = band_input(N, 4 * GRAPH_BATCHES * GRAPH_PER, GRAPH_KINDS, GRAPH_SEED, path)
    steps = (replay + [("set", "signal_debounce", 0, 3), ("set", "peak_threshold", 0, 9.0)] + replay + [("set", "edge_width", None, 1)] + replay +
             [("set", "edge_width", None, 1), ("set", "signal_debounce", 0, 0)] + replay)
    return _case(N, [band], [listener_bins(N, band[2], 10)], steps, GRAPH_SEED, debounce=1, path=path, trace=True)


# -- (7) deferred ----------------------------------------------------------------------------------------------------------
# A deferred batch in mid-cumulation; with its listen half pending the debounce setter is refused, the peak threshold and the
# edge width are accepted and reach the next batch only.
DEFER_SEED = 8700
DEFER_BATCHES = (160, 170, 200)


def case_deferred():
    from parity_tools import listener_bins

    band = band_input(N, sum(DEFER_BATCHES), PATH_KINDS, DEFER_SEED)
    bins = listener_bins(N, band[2], 10)
    pending = [("set", "signal_debounce", 0, 4), ("set", "peak_threshold", 0, 9.0), ("set", "edge_width", None, nine_window_edge(N))]
    steps = [("batch", DEFER_BATCHES[0]), ("set", "signal_debounce", 0, 3),
             ("defer", DEFER_BATCHES[1], [(0, band[2][1], DEFER_BATCHES[0] + 40)], pending), ("batch", DEFER_BATCHES[2])]
    return _case(N, [band], [bins], steps, DEFER_SEED, debounce=1, path="device", trace=True)


# -- the debouncer, re-read ----------------------------------------------------------------------------------------------
class Debouncer:
    """dsp.BoolDebouncer (dsp/dsp.go:139-182), statement by statement.  wrong: None, or one of two debouncers the reach
    test shows the inputs tell apart from the literal one -
      "zeroing"   SetThreshold also clears the state
      "counting"  the pass-through (threshold < 2) keeps counting runs and follows the raw state"""

    def __init__(self, threshold, wrong=None):
        self.threshold, self.wrong = threshold, wrong
        self.effectiveState, self.lastRawState, self.stateCount = False, False, 0

    def set_threshold(self, threshold):
        self.threshold = threshold
        if self.wrong == "zeroing":
            self.effectiveState, self.lastRawState, self.stateCount = False, False, 0

    def debounce(self, rawState):
        rawState = bool(rawState)
        if self.threshold < 2:
            if self.wrong == "counting":
                self.stateCount = 1 if rawState != self.lastRawState else self.stateCount + 1
                self.lastRawState = self.effectiveState = rawState
            return rawState
        if rawState != self.lastRawState:
            self.stateCount = 1
        else:
            self.stateCount += 1
        self.lastRawState = rawState
        if self.stateCount >= self.threshold:
            if rawState != self.effectiveState:
                self.effectiveState = rawState
        return self.effectiveState

    def state(self):
        return self.threshold, int(self.effectiveState), int(self.lastRawState), self.stateCount


def replay_debounce(raw_col, start, first, sets, wrong=None):
    """One listener's raw bits from frame `start` on (its attach; `first` its threshold there) through Debouncer, the
    thresholds of `sets` [(frame, value)] applied in front of their frames: uint8 debounced bits from `start` on."""
    d = Debouncer(first, wrong)
    at = {}
    for f, v in sets:
        at.setdefault(f, []).append(v)
    out = np.zeros(len(raw_col) - start, np.uint8)
    for f in range(start, len(raw_col)):
        for v in at.get(f, ()):
            d.set_threshold(v)
        out[f - start] = d.debounce(raw_col[f])
    return out
