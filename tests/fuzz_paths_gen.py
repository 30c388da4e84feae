"""The seeded generator of tests/test_gpu_fuzz_paths.py (pure numpy: tests/test_fuzz_paths_coverage.py runs it without a
GPU and drives host/batch_plan.h with what it draws).

A seed draws a block size (all eight; the number of frames shrinks as N grows, so that seeds cost about the same), a
sample rate that fits it, a debounce, one to three bands (one or two above N = 16384) with their own tones, strengths,
peak threshold and centre frequency, an edge width (the default, or one of test_scan_segment_geometries' kind: edges of
a few bins, odd edges, nine-window geometries), an input path (parity_case.PATHS), a list of steps - one-frame batches,
batches across cumulation boundaries, at N = 16384 launches of >= 1024 frames x bands that pick k_fft_r32 (with and
without listeners, so with and without its wide tap) and launches that are shorter or hold more than 512 slots
(k_fft_psd<14>), above it batches across frame groups; sdr_attach / sdr_detach between batches and sdr_attach_at inside
deferred ones - and, for a fixed share of the seeds, adversarial frames:
  "silent"        a run of all-zero frames (an idle KiwiSDR), >= 200 frames before the stream ends: -Inf and then NaN
                  in the rolling means and thresholds
  "tied_windows"  frames whose IQ is non-zero only at multiples of P = N / W, W = (N - 2 edge) / 10 the noise window:
                  the psd is exactly W-periodic, every window's ordered sum the same, the first window the reference's
  "tied_peaks"    whole cumulations of frames on the four samples {0, N/4, N/2, 3N/4} with integer spectra whose
                  adjacent bins have equal magnitudes (|(3,4)| = |(5,0)|): exactly tied peak bins (float32 paths)
  "full_scale"    frames of +-32767 and -32768 over every sample (int16 paths)
"""
import numpy as np

from sdrainer_amd import synth

SIZES = (512, 1024, 2048, 4096, 8192, 16384, 32768, 65536)
RATES = {512: 48000, 1024: 96000, 2048: 192000, 4096: 192000, 8192: 2_000_000, 16384: 2_000_000, 32768: 2_000_000, 65536: 4_000_000}
# frames per band, before the geometry's own needs (N = 16384's long launches, silent runs) are added
FRAMES = {512: (500, 900), 1024: (400, 700), 2048: (300, 600), 4096: (260, 480), 8192: (230, 420), 16384: (230, 400),
          32768: (260, 420), 65536: (200, 300)}
PATHS = ("device", "device_sc16", "staged", "staged_sc16", "kiwi", "graph", "graph_sc16")
SC16_PATHS = ("device_sc16", "staged_sc16", "kiwi", "graph_sc16")
KINDS = ("none", "silent", "tied_windows", "tied_peaks", "full_scale")
GRAPH_BATCHES = 6  # sdr_graph_batches(): batches per replay (bank.h RING)
TIED_PEAK_THRESHOLD = 1.0  # the peak threshold of a band of tied-peak frames (dB over the noise floor): the tied pairs are peaks
DEFAULT_SEEDS = 48
# the paths of the first 24 seeds, size by size (seed s: size s % 8, row s // 8): every size with float32 and with int16
# input, every staged format on both sides of N = 16384; later seeds draw theirs
FIRST_PATHS = (("device", "device_sc16", "staged", "staged_sc16", "kiwi", "graph", "graph_sc16", "device"),
               ("staged", "staged_sc16", "kiwi", "graph", "graph_sc16", "device", "staged_sc16", "staged"),
               ("kiwi", "graph", "graph_sc16", "device", "staged", "staged_sc16", "staged", "kiwi"))
FIRST_PATHS = tuple(tuple(row[:5]) + (p16,) + tuple(row[6:]) for row, p16 in zip(FIRST_PATHS, ("device", "graph", "staged_sc16")))


def tied_window(n):
    """(edge, W) with W = (N - 2 edge) / 10 a divisor of N (a nine-window geometry: the reference evaluates windows 0 - 8)."""
    w = n // 16
    return (n - 10 * w) // 2, w


def _edge(rng, n):
    """The default edge, or one of test_scan_segment_geometries' kind."""
    d = synth.default_edge_width(n)
    kind = int(rng.integers(0, 6))
    if kind == 0 or kind == 1:
        return d
    if kind == 2:
        return int(rng.choice([1, 3, 7, 33, 71]))  # edges shorter than a scan piece, windows on odd bins
    if kind == 3:  # nine windows: N - 2 edge a multiple of ten (the reference never evaluates the tenth window)
        return (n - 10 * int(rng.integers(n // 14, n // 10))) // 2
    if kind == 4:
        return int(rng.integers(1, n // 8)) | 1
    return tied_window(n)[0]


def _split(rng, total, n, n_bands, two_long, long_scan=False):
    """Batch lengths that add up to total: one-frame batches, short ones, ones across cumulation boundaries; at N = 16384
    a launch of >= 1024 frames x bands (k_fft_r32 unless more than 512 slots) beside short ones (k_fft_psd<14>); above it
    batches across frame groups (kFft2pGroupMiB of float64 intermediate: 128 MiB / (bands N 16) frames)."""
    out, left = [], total
    if n == 16384:
        big = -(-1024 // n_bands) + int(rng.integers(0, 60))
        first = int(rng.integers(1, 40))
        out += [first, big] + ([big] if two_long else [])
        left = max(0, left - sum(out))
    if long_scan:  # 22 cumulation slots x 3 bands: k_psd_scan deals whole slots (scan_parts 1)
        out.append(2150)
        left -= 2150
    group = (128 << 20) // (n_bands * n * 16) if n > 16384 else 0
    while left > 0:
        r = rng.random()
        if r < 0.15:
            k = 1
        elif r < 0.45:
            k = int(rng.integers(2, 100))
        elif group and r < 0.8:
            k = int(rng.integers(group + 1, 2 * group + 40))
        else:
            k = int(rng.integers(100, 260))
        if n == 16384:
            k = min(k, -(-1024 // n_bands) - 1)  # (short launches: k_fft_psd<14>)
        k = min(k, left)
        out.append(k)
        left -= k
    head, tail = (out[:3 if two_long else 2], out[3 if two_long else 2:]) if n == 16384 else ([], out)
    rng.shuffle(tail)
    return head + tail


class Seed:
    """Everything one seed draws; inputs() makes the frames (host arrays, float32 and int16)."""

    def __init__(self, seed, n=None, path=None, kind=None):
        """n, path, kind: drawn from the seed unless given (the named adversarial cases)."""
        self.seed = seed
        rng = np.random.default_rng(77_000 + seed)
        # the first seeds walk the sizes and the paths (every size with both formats within 16 seeds), later ones draw them
        drawn_n = int(SIZES[seed % len(SIZES)]) if seed < 3 * len(SIZES) else int(rng.choice(SIZES))
        drawn_path = FIRST_PATHS[seed // len(SIZES)][seed % len(SIZES)] if seed < 3 * len(SIZES) else str(rng.choice(PATHS))
        self.n = n = n or drawn_n
        self.rate = RATES[n]
        self.path = path or drawn_path
        sc16 = self.path in SC16_PATHS
        # a fixed share of the seeds: every second one is adversarial, its kind by the input format
        if kind is None:
            kind = "none" if seed % 2 == 0 else ("silent", "tied_windows", "full_scale" if sc16 else "tied_peaks")[(seed // 2) % 3]
        assert kind != "tied_peaks" or not sc16, "tied peak bins need float32 input"
        assert kind != "full_scale" or sc16, "full-scale frames are int16 input"
        self.kind = kind
        self.n_bands = nb = int(rng.integers(1, 4 if n <= 16384 else 3))
        if kind == "tied_windows":
            self.edge = tied_window(n)[0]
        else:
            self.edge = _edge(rng, n)
        # N = 16384 away from graph mode: more than 512 slots (k_fft_psd<14> whatever the launch), or no listener during the
        # first long launch (k_fft_r32 without its wide tap) and one attached before the second (with it); the first 24
        # seeds take one of each
        eager16 = n == 16384 and not self.path.startswith("graph")
        r = seed // len(SIZES) if seed < 3 * len(SIZES) else int(rng.integers(0, 3))
        self.many_slots = eager16 and r == 2
        self.no_listeners_first = eager16 and r != 2
        lo, hi = FRAMES[n]
        total = int(rng.integers(lo, hi))
        if kind == "silent":
            self.silent_len = int(rng.integers(1, 40))
            self.silent_at = int(rng.integers(0, 60))
            total = max(total, self.silent_at + self.silent_len + 200 + int(rng.integers(0, 60)))
        if kind == "tied_peaks":
            total = max(total, 200 + int(rng.integers(0, 80)))  # two whole cumulations of tied frames at least
        self.debounce = int(rng.choice([1, 1, 2, 3, 5]))  # (the bank's: sdr_config signal_debounce)
        self.bands = []
        for b in range(nb):
            weak = bool(rng.random() < 0.3)
            tones = int(rng.integers(1, 13))
            self.bands.append({"tones": tones, "weak": weak, "threshold": float(rng.choice([15.0, 15.0, 12.0, 18.0])),
                               "center": int(rng.integers(3_500, 28_000)) * 1000, "seed": 9_100 + 31 * seed + 7 * b})
        if kind == "tied_peaks":
            self.bands[0]["threshold"] = TIED_PEAK_THRESHOLD
        self.adv_band = int(rng.integers(0, nb)) if kind in ("silent", "tied_windows", "full_scale") else 0
        if self.path.startswith("graph"):
            per = int(rng.integers(1, 60 if n <= 16384 else 40))
            reps = max(2, -(-total // (GRAPH_BATCHES * per)))
            reps = min(reps, 3)
            per = max(per, -(-total // (reps * GRAPH_BATCHES)))
            self.batches = [per] * (reps * GRAPH_BATCHES)
        else:
            long_scan = n <= 1024 and nb == 3
            self.batches = _split(rng, total + (2150 if long_scan else 0), n, nb, self.no_listeners_first, long_scan)
        self.total = sum(self.batches)
        self.rng_state = int(rng.integers(0, 2**31))

    # -- listeners and steps -------------------------------------------------------------------------------------------------
    def steps(self, carriers):
        """The step list of parity_case.Case, and the initial listeners of every band (bins)."""
        rng = np.random.default_rng(self.rng_state)
        n, nb = self.n, self.n_bands
        init, spare = [], []
        for b in range(nb):
            c = list(carriers[b])
            if self.no_listeners_first:
                init.append([])
                spare.append(c + [int(x) for x in rng.integers(0, n, 3)])
                continue
            k = int(rng.integers(0, len(c) + 1))
            init.append(c[:max(1, k)] + ([0, n - 1] if rng.random() < 0.3 else []))
            spare.append(c[max(1, k):] + [int(x) for x in rng.integers(0, n, 2)])
        if self.many_slots:
            b = int(rng.integers(0, nb))
            extra = [int(x) for x in rng.permutation(n)[:520 - len(init[b])]]
            init[b] = init[b] + extra
        graph = self.path.startswith("graph")
        steps, detached, n_lid = [], [set() for _ in range(nb)], [len(x) for x in init]
        pos = 0
        for i, k in enumerate(self.batches):
            # between batches (graph: between replays only)
            quiet = self.no_listeners_first and i <= 2  # (no listener until the first long launch, index 1, is over)
            if self.no_listeners_first and i == 2:
                steps.append(("attach", 0, spare[0].pop(0)))  # (the second long launch, index 2: the wide tap)
                n_lid[0] += 1
            if i > 0 and not quiet and (not graph or i % GRAPH_BATCHES == 0):
                r = rng.random() * (0.45 if graph and i == GRAPH_BATCHES else 1.0)  # (graph: a new capture at least once)
                b = int(rng.integers(0, nb))
                if r < 0.3 and spare[b] and not detached[b]:
                    steps.append(("attach", b, spare[b].pop(0)))
                    n_lid[b] += 1
                elif r < 0.45 and n_lid[b] > len(detached[b]) and i > len(self.batches) // 3:
                    lid = int(rng.choice([x for x in range(n_lid[b]) if x not in detached[b]]))
                    steps.append(("detach", b, lid))
                    detached[b].add(lid)
            if not graph and not quiet and k >= 2 and rng.random() < 0.25:
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

    # -- frames ----------------------------------------------------------------------------------------------------------------
    def inputs(self):
        """[(float32 [total, 2N], int16 [total, 2N] or None, carrier bins)] per band: the frames the bank is given."""
        n, total = self.n, self.total
        rng = np.random.default_rng(self.rng_state + 1)
        out = []
        for b, bd in enumerate(self.bands):
            amp = synth.TONE_AMPLITUDE * (0.0027 if bd["weak"] else 1.0)
            try:
                iq, bins, _ = synth.make_band(total, self.rate, n, bd["tones"], seed=bd["seed"], edge_width=self.edge, amplitude=amp)
            except ValueError:  # (too many tones for a wide edge)
                iq, bins, _ = synth.make_band(total, self.rate, n, 1, seed=bd["seed"], edge_width=self.edge, amplitude=amp)
            q = None
            if self.path in SC16_PATHS:
                q = np.clip(np.rint(iq.astype(np.float64) * (20000.0 / max(1e-9, float(np.max(np.abs(iq)))))), -32768, 32767).astype(np.int16)
            if b == self.adv_band and self.kind != "none":
                q = self._adversarial(rng, iq, q)
            if q is not None:
                iq = (q.astype(np.float32) / np.float32(32767.0)).astype(np.float32)
            out.append((np.ascontiguousarray(iq, np.float32), q, bins))
        return out

    def _adversarial(self, rng, iq, q):
        n, total = self.n, self.total
        if self.kind == "silent":
            a, e = self.silent_at, self.silent_at + self.silent_len
            iq[a:e] = 0.0
            if q is not None:
                q[a:e] = 0
        elif self.kind == "tied_windows":
            _, w = tied_window(n)
            p = n // w
            frames = rng.choice(total, size=max(3, total // 4), replace=False)
            for f in frames:
                if q is not None:
                    row = np.zeros(2 * n, np.int16)
                    v = rng.integers(-12000, 12000, size=(w, 2))
                    row[0::2][::p], row[1::2][::p] = v[:, 0], v[:, 1]
                    q[f] = row
                else:
                    iq[f] = 0.0
                    iq[f, 0::2][::p] = (0.05 * rng.standard_normal(w)).astype(np.float32)
                    iq[f, 1::2][::p] = (0.05 * rng.standard_normal(w)).astype(np.float32)
            self.tied_frames = np.sort(frames)
        elif self.kind == "tied_peaks":
            iq[:] = tied_peak_frames(rng, n, total)
        elif self.kind == "full_scale":
            a = int(rng.integers(0, max(1, total - 30)))
            e = min(total, a + int(rng.integers(3, 25)))
            q[a:e] = rng.choice(np.array([32767, -32767, -32768], np.int16), size=(e - a, 2 * n))
            q[a] = -32768  # (a whole frame of the one value without a positive twin)
        return q


def tied_peak_frames(rng, n, frames):
    """Frames on the samples {0, N/4, N/2, 3N/4} whose spectrum is s * (3 + 4i, 5, 1, i) repeated (s a small integer and a
    quarter turn, drawn per frame): |X| = 5s, 5s, s, s - exactly tied pairs, the psd exactly 4-periodic."""
    X = np.array([3 + 4j, 5, 1, 1j])
    out = np.zeros((frames, 2 * n), np.float32)
    for f in range(frames):
        s = int(rng.integers(1, 9)) * (1j ** int(rng.integers(0, 4)))
        x = np.fft.ifft(X * s)  # quarters of Gaussian integers: exact in float32
        x = np.round(x * 4) / 4
        for m in range(4):
            out[f, 2 * (m * n // 4)] = x[m].real
            out[f, 2 * (m * n // 4) + 1] = x[m].imag
    return out


def family(n):
    """The FFT kernel family of a block size: the 16-point k_fft_psd<log2 N>, N = 16384 (k_fft_psd<14> or k_fft_r32), the
    two-phase k_fft_2p."""
    return "psd" if n <= 8192 else ("16384" if n == 16384 else "2p")


def forced_selection(n_seeds=DEFAULT_SEEDS):
    """Seeds of the default set that between them reach every FFT kernel family, every input path and every adversarial
    kind (tests/test_forced_paths.py runs them under the forced switches)."""
    seeds = [Seed(s) for s in range(n_seeds)]
    want = {("family", f) for f in ("psd", "16384", "2p")} | {("path", p) for p in PATHS} | {("kind", k) for k in KINDS[1:]}
    picked = []
    while want:
        best = max(seeds, key=lambda s: len(want & {("family", family(s.n)), ("path", s.path), ("kind", s.kind)}))
        got = want & {("family", family(best.n)), ("path", best.path), ("kind", best.kind)}
        assert got, f"the default seeds do not reach {sorted(want)}"
        want -= got
        picked.append(best.seed)
    return sorted(picked)
