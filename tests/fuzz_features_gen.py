"""The seeded generator of tests/test_gpu_fuzz_features.py (pure numpy: tests/test_fuzz_features_coverage.py runs it without
a GPU, plans its batches with host/batch_plan.h and runs the oracle alone over its inputs).

Where tests/fuzz_paths_gen.py draws block size, path, band count and listener events over dense float32 and int16 frames,
a seed here draws the features that came later, together:
  format     f32, sc16, cs8 or cu8
  delivery   "device" (dense), "stream" (sdr_process_device_stream*, hop < N, on some seeds a padded band stride), "staged"
             (dense pushes), "staged_hop" (pushes with hop < N: the history the bank keeps on the device), "graph" (dense
             replays), "kiwi" (sc16, dense)
  hop        N, N/2, N/4, N/8 or N/16 where host/overlap.h hop_valid takes it (N = 512 at hop 32 holds one tone)
  windows    one table or None per batch, by transition: "none", "0A" (None -> A), "AB", "A0" (A -> sdr_set_window(NULL)),
             "A0A"; tables of parity_tools.random_window's kind, or the "hard" one (a tenth of the entries exactly 0, a tenth
             negative); graph seeds change the window between replays only
  origin     the first frame: 0, a multiple of 100, or one that puts 2^31 or 2^32 inside the run
  steps      every eager seed holds a one-frame batch, a batch across a cumulation boundary, an attach between batches and a
             deferred batch with sdr_attach_at; with a hop or with trace a sdr_listener_stop, without either a detach and
             ("set", ...) steps of setters_gen's kind
  switches   SDR_FFT_R32=1 at N = 16384 (every k_fft_r32* instance on a few frames), SDR_FFT_FPW=2 / 4 on float32 seeds of
             512 or 1024 points with a batch long enough for the multi-frame workgroup (fft_frames_per_wg's rule); one seed
             of the table reaches k_fft_r32_hop_sc16 by the plan's own rule (342 frames x 3 bands at hop 2048)
  kind       every third seed is adversarial, by its format: "silent" (exact zeros over a run of samples cut at no multiple
             of the hop, >= 200 frames behind it: f32, sc16, cs8), "full_scale" (sc16: 32767 / -32767 / -32768 and one frame
             of -32768 only; cs8: 127 / -128 and one frame of -128; cu8: 0 / 255 and one frame of 0); every 8-bit stream
             holds iq8_tools.plant_all_bytes in its first frames
The first 32 seeds walk TABLE, later ones draw.  A seed with a hop runs with trace; so does every fourth dense one."""
import numpy as np

import iq8_tools
from parity_tools import listener_bins, make_stream, random_window
from sdrainer_amd import synth

SIZES = (512, 1024, 2048, 4096, 8192, 16384, 32768, 65536)
RATES = iq8_tools.RATE
FORMATS = ("f32", "sc16", "cs8", "cu8")
DELIVERIES = ("device", "stream", "staged", "staged_hop", "graph", "kiwi")
TRANSITIONS = ("none", "0A", "AB", "A0", "A0A")
KINDS = ("none", "silent", "full_scale")
# frames per band: fewer as N grows; a seed with a hop runs with trace and stays below 600
FRAMES = {512: (400, 590), 1024: (350, 590), 2048: (300, 550), 4096: (260, 480), 8192: (230, 420), 16384: (230, 400),
          32768: (220, 330), 65536: (180, 250)}
GRAPH_BATCHES = 6  # sdr_graph_batches()
R32_OWN_RULE = 342  # frames of a three-band batch at N = 16384: 1026 frames x bands, k_fft_r32 by fft_choice's own rule
O31, O32 = 1 << 31, 1 << 32
DEFAULT_SEEDS = 48
_D, _S, _T, _H, _G, _K = DELIVERIES
# (N, format, delivery, N / hop, window transition, hard table, origin: 0 | "100" | "31" | "32", switch: None | "r32" | "fpw2" |
# "fpw4" | "own"): what the first seeds take, chosen for tests/test_fuzz_features_coverage.py
TABLE = (
    (512, "f32", _D, 1, "none", False, 0, "fpw2"),
    (1024, "f32", _T, 1, "AB", False, "100", "fpw4"),
    (2048, "f32", _S, 4, "0A", True, 0, None),
    (4096, "sc16", _D, 1, "A0", False, 0, None),
    (8192, "cs8", _S, 8, "A0A", False, "31", None),
    (512, "sc16", _H, 16, "none", False, 0, None),
    (1024, "cu8", _H, 2, "0A", False, "32", None),
    (2048, "cs8", _T, 1, "A0", True, 0, None),
    (16384, "sc16", _S, 8, "none", False, 0, "own"),
    (16384, "f32", _D, 1, "0A", False, 0, "r32"),
    (16384, "sc16", _T, 1, "A0A", True, "100", "r32"),
    (16384, "cs8", _D, 1, "A0", False, 0, "r32"),
    (16384, "f32", _H, 4, "none", False, 0, "r32"),
    (16384, "cu8", _S, 16, "0A", False, 0, "r32"),
    (32768, "cs8", _H, 2, "AB", False, 0, None),
    (65536, "cs8", _S, 16, "none", False, 0, None),
    (32768, "f32", _G, 1, "AB", False, 0, None),
    (65536, "cu8", _T, 1, "A0", True, 0, None),
    (32768, "sc16", _G, 1, "A0", False, "100", None),
    (32768, "f32", _H, 8, "none", False, 0, None),
    (4096, "cs8", _G, 1, "none", False, 0, None),
    (8192, "cu8", _G, 1, "0A", False, 0, None),
    (2048, "sc16", _K, 1, "none", False, "100", None),
    (1024, "cu8", _D, 1, "AB", True, 0, None),
    (8192, "sc16", _H, 4, "A0", False, "31", None),
    (512, "cu8", _S, 16, "0A", True, 0, None),
    (4096, "f32", _T, 1, "none", False, 0, None),
    (65536, "sc16", _S, 16, "AB", False, 0, None),
    (16384, "cu8", _H, 8, "A0", False, 0, "r32"),
    (2048, "cs8", _D, 1, "none", False, 0, None),
    (32768, "cu8", _G, 1, "none", False, 0, None),
    (1024, "sc16", _T, 1, "0A", False, "100", None),
)


def family(n):
    """The FFT kernel family of a block size (fuzz_paths_gen.family)."""
    return "psd" if n <= 8192 else ("16384" if n == 16384 else "2p")


def hop_valid(hop, n):
    """host/overlap.h hop_valid, for hop > 0."""
    return 32 <= hop <= n and hop & (hop - 1) == 0 and hop * 16 >= n


def frames_per_wg(fpw, frames, n_bands):
    """host/batch_plan.h fft_frames_per_wg."""
    while fpw > 1 and -(-frames // fpw) * n_bands < 256:
        fpw //= 2
    return fpw


def hard_window(n, seed):
    """random_window's kind with about a tenth of the entries exactly 0 and about a tenth negated: no NaN, no Inf."""
    w = random_window(n, seed)
    r = np.random.default_rng(seed + 1).random(n)
    w[r < 0.1] = 0.0
    w[r > 0.9] *= np.float32(-1.0)
    return w


def _draw_table_row(rng):
    n = int(rng.choice(SIZES))
    fmt = str(rng.choice(FORMATS))
    deliveries = [d for d in DELIVERIES if d != _K or fmt == "sc16"]
    delivery = str(rng.choice(deliveries))
    div = 1
    if delivery in (_S, _H):
        div = int(rng.choice([d for d in (2, 4, 8, 16) if hop_valid(n // d, n)]))
    trans = str(rng.choice(TRANSITIONS))
    origin = [0, 0, "100", "31", "32"][int(rng.integers(0, 5))]
    switch = None
    if n == 16384 and rng.random() < 0.4:
        switch = "r32"
    elif n <= 1024 and fmt == "f32" and delivery in (_D, _T) and rng.random() < 0.5:
        switch = ("fpw2", "fpw4")[int(rng.integers(0, 2))]
    return n, fmt, delivery, div, trans, bool(rng.random() < 0.25), origin, switch


class Seed:
    """Everything one seed draws; inputs() makes the streams, steps() the step list of parity_case.Case."""

    def __init__(self, seed):
        self.seed = seed
        rng = np.random.default_rng(91_000 + seed)
        row = TABLE[seed] if seed < len(TABLE) else _draw_table_row(rng)
        self.n, self.fmt, self.delivery, div, self.transition, self.hard, origin, self.switch = row
        n = self.n
        self.rate = RATES[n]
        self.hop = n // div
        assert hop_valid(self.hop, n) and (div == 1) == (self.delivery not in (_S, _H))
        self.graph = self.delivery == _G
        self.path = {_D: "device", _S: "device", _T: "staged", _H: "staged", _G: "graph"}.get(self.delivery, "kiwi")
        if self.delivery != _K and self.fmt != "f32":
            self.path += "_" + self.fmt
        self.iq8 = {"cs8": iq8_tools.CS8, "cu8": iq8_tools.CU8}.get(self.fmt)
        self.env = {"r32": {"SDR_FFT_R32": 1}, "fpw2": {"SDR_FFT_FPW": 2}, "fpw4": {"SDR_FFT_FPW": 4}}.get(self.switch, {})
        fpw = self.env.get("SDR_FFT_FPW", 0)
        self.trace = self.hop < n or (seed % 4 == 1 and not fpw)
        self.timed = self.trace
        self.kind = "none"
        if seed % 3 == 2:  # every third seed is adversarial, its kind by the format
            self.kind = {"f32": "silent", "cu8": "full_scale"}.get(self.fmt, ("silent", "full_scale")[(seed // 3) % 2])
        self.n_bands = nb = 3 if self.switch == "own" else int(rng.integers(1, 4 if n <= 16384 else 3))
        self.tones = 1 if self.hop < 64 else 2
        self.pad = int(rng.choice([0, 40, 104])) if self.delivery == _S else 0
        self.debounce = int(rng.choice([1, 1, 2, 3]))
        lo, hi = FRAMES[n]
        total = int(rng.integers(lo, hi))
        # a batch long enough for the plan to take the kernel the switch (or the plan's own rule) is about
        big = 0
        if fpw:
            big = max(515, fpw * -(-256 // nb)) + int(rng.integers(0, 20))
            assert frames_per_wg(fpw, big, nb) == fpw
        elif self.switch == "own":
            big = R32_OWN_RULE + int(rng.integers(0, 10))
        total = max(total, big + 60)
        if self.kind == "silent":
            # zeros over [silent_at, silent_at + silent_len) samples: cut at no multiple of the hop, at least one whole frame
            tight = self.hop == 65536  # (dense frames of 65536 points: 256 of them are 2^24 samples)
            self.silent_at = self.hop * int(rng.integers(14 if tight else 20, 24 if tight else 60)) + 1 + 2 * int(rng.integers(0, self.hop // 2))
            self.silent_len = n + self.hop * int(rng.integers(1, 6)) + int(rng.integers(0, self.hop))
            behind = -(-(self.silent_at + self.silent_len) // self.hop)  # the first frame that holds no zeroed sample
            total = max(total, behind + 200 + int(rng.integers(0, 20 if tight else 40)))
            self.silent_behind = behind
        if self.kind == "full_scale":
            self.full_at = int(rng.integers(130, total - 40))  # (frames: the oracle has seen a cumulation by then)
            self.full_len = (n * int(rng.integers(3, 6))) if self.hop == n else n + self.hop * int(rng.integers(3, 20))
        if self.graph:
            reps = 3 if self.transition == "A0A" else int(rng.integers(2, 4))
            per = max(1, -(-total // (reps * GRAPH_BATCHES)))
            if n == 65536:
                per = min(per, 256 // (reps * GRAPH_BATCHES))
            self.batches = [per] * (reps * GRAPH_BATCHES)
        else:
            self.batches = self._split(rng, total, big)
        self.total = sum(self.batches)
        assert (self.total - 1) * self.hop + n <= 1 << 24, "a band's stream above 2^24 samples"
        assert not self.trace or self.total <= 640, "a traced seed holds about 600 frames at the most"
        self.adv_band = int(rng.integers(0, nb))
        self.first_frame = self._origin(rng, origin)
        self.windows, self.tables = self._windows(rng)
        self.band_seeds = [13_100 + 31 * seed + 7 * b for b in range(nb)]
        self.rng_state = int(rng.integers(0, 2**31))

    # -- what the seed decides before any sample exists -------------------------------------------------------------------------
    def _split(self, rng, total, big):
        """Batch lengths: the long one (if any) first, a one-frame batch, one of 101 - 180 frames (across a cumulation
        boundary wherever it starts), then short and middling ones."""
        out, left = [1, int(rng.integers(101, 131))], total - big
        left -= sum(out)
        while left > 0:
            k = int(rng.integers(2, 60)) if rng.random() < 0.4 else int(rng.integers(60, 200))
            k = min(k, left)
            out.append(k)
            left -= k
        rng.shuffle(out)
        return ([big] if big else []) + [int(x) for x in out]

    def _origin(self, rng, origin):
        if origin in (0, "100"):
            return 0 if origin == 0 else 100 * int(rng.integers(1, 40_000_000))
        # the crossing inside the run, away from its ends: 2^31 = 48, 2^32 = 96 modulo 100
        edge = O31 if origin == "31" else O32
        c = (48 if origin == "31" else 96) + 100 * int(rng.integers(0, max(1, (self.total - 60) // 100)))
        assert 0 < c < self.total and (edge - c) % 100 == 0
        return edge - c

    def crossing(self):
        """The stream frame whose bank frame index is a multiple of 2^31, or None."""
        c = (-self.first_frame) % O31
        return c if self.first_frame and c < self.total else None

    def _windows(self, rng):
        """One table or None per batch, and the tables by name."""
        n, nbat = self.n, len(self.batches)
        mk = hard_window if self.hard else random_window
        A, B = mk(n, 50_000 + 2 * self.seed), mk(n, 50_001 + 2 * self.seed)
        phases = {"none": [None], "0A": [None, A], "AB": [A, B], "A0": [A, None], "A0A": [A, None, A]}[self.transition]
        unit = GRAPH_BATCHES if self.graph else 1
        slots = nbat // unit
        assert slots >= len(phases), "fewer batches (replays) than windows"
        cuts = sorted(int(x) for x in rng.choice(np.arange(1, slots), size=len(phases) - 1, replace=False)) if len(phases) > 1 else []
        out = []
        for i in range(slots):
            out += [phases[sum(1 for c in cuts if c <= i)]] * unit
        return out, {"A": A, "B": B}

    # -- listeners and steps --------------------------------------------------------------------------------------------------
    def steps(self, carriers):
        """(steps, initial listener bins per band)."""
        rng = np.random.default_rng(self.rng_state)
        n, nb = self.n, self.n_bands
        init, spare = [], []
        for b in range(nb):
            bins = listener_bins(n, carriers[b], 3 * len(carriers[b]) + 2)
            keep = int(rng.integers(1, len(carriers[b]) + 1))  # (the other carriers wait for an attach or an sdr_attach_at)
            init.append(bins[:keep] + ([0, n - 1] if rng.random() < 0.3 else []))
            spare.append(bins[keep:3 * len(carriers[b])])
        nbat = len(self.batches)
        steps, n_lid, detached = [], [len(x) for x in init], [set() for _ in range(nb)]
        if self.graph:
            for i, k in enumerate(self.batches):
                if i and i % GRAPH_BATCHES == 0:
                    b = int(rng.integers(0, nb))
                    r = rng.random()
                    if r < 0.6 and spare[b] and not detached[b]:
                        steps.append(("attach", b, spare[b].pop(0)))
                        n_lid[b] += 1
                    elif r < 0.8 and not self.timed:
                        lid = int(rng.integers(0, n_lid[b]))
                        if lid not in detached[b]:
                            steps.append(("detach", b, lid))
                            detached[b].add(lid)
                steps.append(("batch", k))
            return steps, init
        # eager: one deferred batch with sdr_attach_at (not the first batch, two frames at least), an attach and a stop (or,
        # untimed, a detach) at boundaries of their own, then whatever else is drawn
        defer_at = int(rng.choice([i for i in range(1, nbat) if self.batches[i] >= 2]))
        attach_before = int(rng.integers(1, nbat))
        stop_before = int(rng.integers(1, nbat))
        pos, peaks_off = 0, False
        for i, k in enumerate(self.batches):
            if i:
                b = int(rng.integers(0, nb))
                r = rng.random()
                if peaks_off:  # (the peak search is off for one batch at the most)
                    steps.append(("set", "find_peaks", None, True))
                    peaks_off = False
                if (i == attach_before or r < 0.2) and spare[b] and not detached[b]:
                    steps.append(("attach", b, spare[b].pop(0)))
                    n_lid[b] += 1
                if self.timed and (i == stop_before or r > 0.85):
                    steps.append(("stop", b, int(rng.integers(0, len(init[b])))))  # (an initial listener: it has taken a frame)
                if not self.timed:
                    if (i == stop_before or r > 0.85) and i > nbat // 3 and n_lid[b] > len(detached[b]) + 1:
                        lid = int(rng.choice([x for x in range(n_lid[b]) if x not in detached[b]]))
                        steps.append(("detach", b, lid))
                        detached[b].add(lid)
                    if 0.3 < r < 0.6:
                        steps.append(self._set(rng))
                        peaks_off = steps[-1][1] == "find_peaks"
            if i == defer_at or (k >= 2 and i and rng.random() < 0.15):
                late = []
                for _ in range(int(rng.integers(1, 4))):
                    b = int(rng.integers(0, nb))
                    if spare[b] and not detached[b]:
                        late.append((b, spare[b].pop(0), pos + int(rng.integers(0, k))))
                        n_lid[b] += 1
                steps.append(("defer", k, sorted(late, key=lambda t: t[2])))
            else:
                steps.append(("batch", k))
            pos += k
        return steps, init

    def _set(self, rng):
        """A ("set", ...) step of setters_gen's kind."""
        which = int(rng.integers(0, 4))
        b = int(rng.integers(0, self.n_bands))
        if which == 0:
            return ("set", "peak_threshold", b, float(rng.choice([9.0, 12.0, 18.0, 21.5])))
        if which == 1:
            return ("set", "signal_debounce", b, int(rng.choice([0, 1, 2, 3, 5])))
        if which == 2:
            nine = (self.n - 10 * (self.n // 16)) // 2  # (fuzz_paths_gen.tied_window: nine windows)
            return ("set", "edge_width", None, int(rng.choice([1, nine, synth.default_edge_width(self.n)])))
        return ("set", "find_peaks", None, False)

    # -- streams --------------------------------------------------------------------------------------------------------------
    def inputs(self):
        """[(float32 stream [samples, 2], what the path sends or None, carrier bins)] per band."""
        n, hop, total = self.n, self.hop, self.total
        rng = np.random.default_rng(self.rng_state + 1)
        out = []
        for b in range(self.n_bands):
            if self.iq8 is not None:
                q, bins = iq8_tools.stream(n, hop, total, self.tones, self.band_seeds[b], self.iq8)
                q = np.ascontiguousarray(q)
                if hop < 512:  # (plant_all_bytes needs 512 samples for its 256 places: the stream's first 512-sample rows)
                    for p in range(min(iq8_tools.POOL, q.shape[0] // 512)):
                        iq8_tools.plant_all_bytes(q.reshape(-1)[p * 1024:(p + 1) * 1024], p)
            else:
                s, q, bins = make_stream(n, hop, total, self.rate, self.tones, self.band_seeds[b], self.fmt == "sc16")
                s = np.array(s, np.float32)
            if b == self.adv_band and self.kind != "none":
                x = s if q is None else q
                if self.kind == "silent":
                    x[self.silent_at:self.silent_at + self.silent_len] = 0
                else:
                    a = self.full_at * hop
                    vals = {"sc16": [32767, -32767, -32768], "cs8": [127, -128], "cu8": [0, 255]}[self.fmt]
                    x[a:a + self.full_len] = rng.choice(np.array(vals, x.dtype), size=(self.full_len, 2))
                    x[a + (self.full_len - n):a + self.full_len] = vals[0] if self.fmt == "cu8" else vals[-1]  # one whole frame of the one value
            if self.iq8 is not None:
                s = iq8_tools.to_f32(q, self.iq8)
            elif q is not None:
                s = (q.astype(np.float32) / np.float32(32767.0)).astype(np.float32)
            out.append((np.ascontiguousarray(s, np.float32), q, bins))
        return out

    def full_frames(self):
        """(first frame, frames) that lie wholly in the full-scale run, and the frame of the one value."""
        count = (self.full_len - self.n) // self.hop + 1
        return self.full_at, count, self.full_at + count - 1

    def ident(self):
        o = self.first_frame
        origin = "0" if not o else ("x31" if self.crossing() is not None and (o + self.crossing()) == O31 else
                                    "x32" if self.crossing() is not None else f"at{o}")
        sw = f"-{self.switch}" if self.switch else ""
        return (f"seed{self.seed:03d}-{self.n}-{self.fmt}-{self.delivery}-hop{self.hop}-w{self.transition}{'-hard' if self.hard else ''}"
                f"-{origin}-{self.kind}{'-trace' if self.trace else ''}{sw}")


def case_of(s, bands=None):
    """The parity_case.Case of seed s (and its input bands)."""
    from parity_case import Case

    bands = bands or s.inputs()
    steps, init = s.steps([bd[2] for bd in bands])
    case = Case(s.n, s.n_bands, None, 0, steps, seed=s.seed, rate=s.rate, debounce=s.debounce, path=s.path, bands=bands, init_bins=init,
                nan_ok=s.kind == "silent", hop=s.hop if s.hop < s.n else None, pad=s.pad, windows=s.windows, trace=s.trace,
                first_frame=s.first_frame)
    return case, bands
