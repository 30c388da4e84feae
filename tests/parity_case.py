"""One bank's stream against the CPU oracle, bit for bit: the `Case` driver every GPU parity test shares (a plain helper
module, not a test file; what it is built from is in tests/parity_tools.py).

A Case holds n_bands bands of keyed carriers and a list of steps; it runs one oracle receiver per band, attached and
detached at the bank's frames and stitched into one stream per band (a listener's keying column is zero before it is
attached), and compares with what sdr_poll delivers and what stays on the device: frame records, keying bits, edges,
runes, decoder state, the exact cumulation rows (and the kept row: never below the exact one, equal at and beside every
peak, those beyond the bank's max_peaks included), peaks with their frequencies (the oracle's first max_peaks of a
cumulation, and the number of runs it found), and drop counters of 0.

The input reaches the bank by one of the paths of include/sdrainer_hip.h:
  "device"       float32 in device memory (sdr_process_device)
  "device_sc16"  complex int16 in device memory (sdr_process_device_sc16)
  "device_cs8", "device_cu8"  complex 8-bit, signed / unsigned, in device memory (sdr_process_device_iq8)
  "staged"       float32 from the host (sdr_push_iq -> sdr_process_staged)
  "staged_sc16"  complex int16 from the host (sdr_push_iq_sc16)
  "staged_cs8", "staged_cu8"  complex 8-bit from the host (sdr_push_iq8)
  "kiwi"         KiwiSDR SND payloads, big-endian int16 (sdr_push_kiwi_snd), a batch's frames in several messages
  "graph"        hipGraph replays of float32 batches (sdr_graph_capture / sdr_graph_launch)
  "graph_sc16"   the same for sc16 (sdr_graph_capture_sc16 / sdr_graph_launch_sc16)
  "graph_cs8", "graph_cu8"  the same for 8-bit input (sdr_graph_capture_iq8 / sdr_graph_launch_iq8)
The oracle always reads the float32 values the bank was given: for sc16 and KiwiSDR input float32(x) / 32767, for 8-bit
input iq8_tools.to_f32.

With a hop below the block size frame f of a band is stream[f * hop : f * hop + N]: the oracle is fed the materialised
frames, the device paths go through sdr_process_device_stream(_sc16) with the pointer advanced by frames * hop, the staged
paths push the samples each batch adds, and what means time follows the hop (parity_tools.decode).  With a window per
batch the oracle is fed the frames times the window in float32 (parity_tools.windowed).
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from iq8_tools import to_f32 as iq8_to_float32
from oracle import oracle as orc
from sdrainer_amd import synth
from parity_tools import (RATES, REC_FIELDS, bits_equal, check_batch_polled, check_device_batch, decode, frames32, frames_of, listener_bins,
                          make_stream, nan_equal_bits, sc16_to_float32, windowed)

RATE = 2_000_000
PATHS = ("device", "device_sc16", "device_cs8", "device_cu8", "staged", "staged_sc16", "staged_cs8", "staged_cu8", "kiwi", "graph",
         "graph_sc16", "graph_cs8", "graph_cu8")
SC16_PATHS = ("device_sc16", "staged_sc16", "kiwi", "graph_sc16")
IQ8_PATHS = {"device_cs8": 0, "device_cu8": 1, "staged_cs8": 0, "staged_cu8": 1, "graph_cs8": 0, "graph_cu8": 1}  # -> SDR_IQ8_CS8 / SDR_IQ8_CU8
SETTERS = ("peak_threshold", "edge_width", "signal_debounce", "find_peaks")
KIWI_HEADER = bytes([0x01] + [7] * 16)  # the 17 bytes in front of an SND message's samples (flags, sequence, smeter)


def _extra_bins(n, carriers, count, seed):
    """`count` listener bins besides the keyed carriers: 0 and N - 1, a carrier twice, both neighbours of every fourth
    carrier, then noise bins (seeded)."""
    carriers = [int(c) for c in carriers]
    out = [0, n - 1, carriers[0]]
    for c in carriers[::4]:
        out += [c - 1, c + 1]
    taken = set(carriers) | set(out)
    rng = np.random.default_rng(seed)
    noise = rng.permutation([b for b in range(n) if b not in taken])
    out += [int(b) for b in noise[:max(0, count - len(out))]]
    assert len(out) >= count, "not enough bins"
    return out[:count]


def _per_band(v, n_bands):
    return list(v) if isinstance(v, (list, tuple)) else [v] * n_bands


def _refused(s):
    """A ("set", ...) step whose value is ("bad", value): the bank must refuse it."""
    return isinstance(s[3], tuple) and s[3][0] == "bad"


class Case:
    """One bank's stream: bands of keyed carriers, the listeners attached before the first frame, then a list of steps
       ("batch", frames)                      an eager batch
       ("defer", frames, [(band, bin, s)])    a deferred batch; after its peaks, sdr_attach_at(band, bin, s) in order
       ("attach", band, bin) / ("detach", band, lid)   between batches
       ("stop", band, lid)                    sdr_listener_stop between batches (with a hop or with trace: the hop-timed
                                              decoder is stopped there, and what it writes is stamped with the frame before)
       ("set", name, band, value)             a control between two batches, on the bank and on the oracle(s): name is
                                              "peak_threshold" or "signal_debounce" (band: the band), "edge_width" or
                                              "find_peaks" (band: None, the bank's).  A value the bank must refuse is
                                              ("bad", value): SDR_ERR_BAD_ARG is expected and the oracle is not told.
                                              After every accepted "edge_width", and before the next batch,
                                              sdr_read_frame_records of the batch just finished must return SDR_OK and
                                              the oracle's records - those of the width the batch ran with
    A deferred batch takes a fourth element, a list of ("set", ...) steps called while its listen half is pending: the
    bank must refuse "signal_debounce" there (SDR_ERR_STATE, the oracle is not told) and accept the others, which reach the
    next batch only (the oracle is told behind the deferred batch's last frame).
    (steps may also be a function of the carriers' bins per band, which exist once the input does)

    Per band (a value, or a list with one per band): peak threshold and centre frequency.  The sample rate, the edge width
    and the debounce are the bank's (sdr_config), one for all of its bands: sdr_set_signal_debounce reaches only the
    listeners attached at the time, as the reference's Receiver.SetSignalDebounce does, and every later listener starts
    from the bank's value.  `bands` replaces the synthetic carriers: one
    (float32 stream [samples, 2] or its dense frames [total, 2N], int16 of the same shape or None, carrier bins) per band -
    the int16 array is what the sc16 and KiwiSDR paths send, and the float32 one must then be its value (sc16_to_float32).
    Graph paths take batches of one length, sdr_graph_batches() of them per replay, with attach, detach and a new window
    only between replays (each one is followed by a release and a new capture); no deferred batches.  A "set" between
    replays is called with the capture in place: the next replay runs without a new capture, except behind an "edge_width"
    or "find_peaks" that changed the value - then sdr_graph_launch must refuse (SDR_ERR_STATE) and a release and a new
    capture follow.  nan_ok: the oracle's
    stream holds NaN (a silent run: -Inf and then NaN in the rolling means and thresholds), and NaN compares by class in
    the float fields.

    hop: samples between frame starts (None or 0: dense frames); KiwiSDR and graph input take no hop below N, as the
    library refuses it.  pad: samples behind every band's stream in device memory (the band stride of the stream calls).
    windows: one table or None per batch; the bank is told only when it changes.  trace: the bank is created with
    trace=True, and every checked batch is also held to the oracle's traced values, raw and debounced bits
    (sdr_read_trace) and to the psd and dB rows of the frames spectrum_frames() names.  With a hop or with trace the
    expected text, decoder state and rune frames are the hop-timed decoder's over the oracle's debounced bits, and every
    step is a batch, a deferred batch or an attach (no detach): a late listener's decoder ticks from the frame it was attached
    at, and its tap is compared from that frame on.

    The staged paths with a hop below N (the sample range of _enqueue) are run by tests/test_gpu_fuzz_features.py's default
    seeds 5, 6, 12, 14, 19, 24 and 28, one per format and kernel family at least; run_graph with windows (a window set before
    the capture, release and a new capture when the next replay's window differs) by its seeds 16, 18 and 21.

    first_frame: the bank frame index of the stream's first frame (sdr_set_first_frame before the first attach; a multiple
    of 100).  Steps, spans and the oracle stay counted from 0; every frame number the bank hands out is expected shifted by
    it - first_frame, chunk frames and total_frames as int64, edge and rune frames modulo 2^32 - and sdr_attach_at is given
    shifted start frames.  frame_in_batch and whatever is no frame number are what they are at 0."""

    def __init__(self, n, n_bands, carriers, listeners, steps, seed, rate=RATE, free_last=True, max_listeners=None, total_frames=None,
                 *, edge=None, debounce=1, threshold=15.0, centers=None, path="device", bands=None, init_bins=None, max_peaks=1024,
                 nan_ok=False, hop=None, pad=0, windows=None, trace=False, first_frame=0):
        assert path in PATHS, path
        assert first_frame >= 0 and first_frame % 100 == 0, "the first frame is a multiple of the cumulation size"
        self.first_frame = first_frame
        self.n, self.n_bands, self.rate, self.path, self.nan_ok = n, n_bands, rate, path, nan_ok
        self.hop, self.step, self.pad, self.trace = hop or 0, hop or n, pad, trace
        assert self.step == n or path.startswith("device") or path.startswith("staged"), f"{path} input takes no hop below N"
        assert not pad or (self.hop and path.startswith("device")), "a padded band stride is the device stream calls'"
        self.timed = bool(self.hop or trace)
        self.edge = synth.default_edge_width(n) if edge is None else edge
        self.debounce, self.threshold = debounce, _per_band(threshold, n_bands)
        self.total = total_frames or sum(s[1] for s in steps if s[0] in ("batch", "defer"))
        self.centers = [14000000 + 100000 * b for b in range(n_bands)] if centers is None else _per_band(centers, n_bands)
        self.max_peaks = max_peaks
        samples = (self.total - 1) * self.step + n
        self.stream, self.q, self.carriers, self.init_bins, made = [], [], [], [], []
        for b in range(n_bands):
            if bands is None:
                iq, bins, _ = synth.make_band_torch(self.total, rate, n, carriers, seed=seed + 17 * b, device="cuda", free_last_window=free_last)
                made.append(iq.view(-1, 2))
                self.stream.append(iq.cpu().numpy().reshape(-1, 2))
                self.q.append(None)
            else:
                f32, q, bins = bands[b]
                assert f32.size == 2 * samples and f32.dtype == np.float32, f"band {b}: not {self.total} frames of float32"
                if path in SC16_PATHS:
                    assert q is not None and bits_equal(sc16_to_float32(q), f32), f"band {b}: the float32 input is not its int16's value"
                if path in IQ8_PATHS:
                    assert q is not None and bits_equal(iq8_to_float32(q, IQ8_PATHS[path]), f32), f"band {b}: the float32 input is not its bytes' value"
                self.stream.append(f32.reshape(-1, 2))
                self.q.append(None if q is None else q.reshape(-1, 2))
            self.carriers.append([int(x) for x in bins])
            if init_bins is not None:
                self.init_bins.append([int(x) for x in init_bins[b]])
            else:
                self.init_bins.append((self.carriers[b] + _extra_bins(n, bins, max(0, listeners - len(bins)), seed + 17 * b))[:listeners])
        if made:
            import torch

            self._dev = torch.stack(made)  # (twice the input on the device until `made` goes)
            del made
        self.steps = steps = steps(self.carriers) if callable(steps) else steps
        self.spans, pos = [], 0  # the batches' frames [a, e)
        for s in steps:
            if s[0] in ("batch", "defer"):
                self.spans.append((pos, pos + s[1]))
                pos += s[1]
        assert self.total == pos, f"the steps hold {pos} frames, not {self.total}"
        assert not self.timed or all(s[0] != "detach" for s in steps), "with a hop or with trace no listener is detached"
        self.windows = [None] * len(self.spans) if windows is None else list(windows)
        assert len(self.windows) == len(self.spans), "one window (or None) per batch"
        self.max_frames = max(e - a for a, e in self.spans)
        late = sum(1 for s in steps if s[0] == "attach") + sum(len(s[2]) for s in steps if s[0] == "defer")
        self.max_listeners = max_listeners or max(1, max(len(b) for b in self.init_bins) + late)  # (a reused slot needs none: an upper bound)
        # every listener of every band: (attached at frame, detached at frame or None)
        self.life = [[(0, None) for _ in bins] for bins in self.init_bins]
        self.bins = [list(bins) for bins in self.init_bins]
        # ... and the bank's id of each: the lowest free slot at its attach (ListenerPool.BindNext), so a listener attached
        # behind a detach reuses an id, while the oracle numbers its listeners as they come; heir: the listener that took
        # its slot over, or None
        self.stops = {}  # (band, listener): the frames in front of which it is stopped
        self.slot = [list(range(len(bins))) for bins in self.init_bins]
        self.heir = [[None] * len(bins) for bins in self.init_bins]
        free = [[] for _ in self.init_bins]

        def bind(band, bn, at):
            self.bins[band].append(bn)
            self.life[band].append((at, None))
            self.heir[band].append(None)
            if free[band]:
                sl = min(free[band])
                free[band].remove(sl)
                owner = max(i for i, x in enumerate(self.slot[band]) if x == sl)
                self.heir[band][owner] = len(self.slot[band])
            else:
                sl = len(set(self.slot[band]))
            self.slot[band].append(sl)
        pos = 0
        for s in steps:
            if s[0] == "attach":
                bind(s[1], s[2], pos)
            elif s[0] == "detach":
                self.life[s[1]][s[2]] = (self.life[s[1]][s[2]][0], pos)
                free[s[1]].append(self.slot[s[1]][s[2]])
            elif s[0] == "stop":
                assert self.timed and pos > self.life[s[1]][s[2]][0], "a stop needs the hop-timed decoders, behind the listener's first frame"
                self.stops.setdefault((s[1], s[2]), []).append(pos)
            elif s[0] == "set":
                assert s[1] in SETTERS and (s[2] is None) == (s[1] in ("edge_width", "find_peaks")), f"no such control: {s}"
            else:
                for band, bn, at in s[2] if s[0] == "defer" else []:
                    assert pos <= at <= pos + s[1], f"band {band}: attach_at frame {at} outside its batch (or the frame behind it)"
                    bind(band, bn, at)
                pos += s[1]
        # While no attach follows a detach on a band - every caller from before slots were reused - the bank's ids are the
        # oracle's and nobody has an heir: gone(), check_end and every attach and detach then do what they always did.
        reused = any(h is not None for heirs in self.heir for h in heirs)
        assert reused or all(sl == list(range(len(sl))) for sl in self.slot), "without a reused slot the ids are the oracle's"

    @classmethod
    def of_streams(cls, n, hop, calls, n_bands, tones, listeners, sc16, seed, windows=None, pad=0):
        """Device-resident streams of keyed carriers (parity_tools.make_stream) in calls of `calls` frames, the listeners on
        the carriers and beside them (listener_bins), on a bank with trace."""
        made = [make_stream(n, hop or n, sum(calls), RATES[n], tones, seed + 17 * b, sc16) for b in range(n_bands)]
        return cls(n, n_bands, None, 0, [("batch", x) for x in calls], seed, rate=RATES[n], max_listeners=listeners,
                   path="device_sc16" if sc16 else "device", bands=made, init_bins=[listener_bins(n, m[2], listeners) for m in made],
                   hop=hop, pad=pad, windows=windows, trace=True)

    def frames(self, b, a, e):
        """Frames [a, e) of band b as the oracle is fed them: float32 [frames, 2N], each batch's times that batch's window."""
        n = self.n
        f = frames_of(self.stream[b], n, self.hop, a, e) if self.hop else self.stream[b][a * n:e * n].reshape(-1, 2 * n)
        out = None
        for (lo, hi), w in zip(self.spans, self.windows):
            lo, hi = max(a, lo), min(e, hi)
            if w is not None and lo < hi:
                out = np.array(f) if out is None else out
                out[lo - a:hi - a] = windowed(f[lo - a:hi - a], w, n)
        return f if out is None else out

    def oracle_input(self, b):
        """The float32 frames band b is given, host side."""
        return self.frames(b, 0, self.total)

    def spectrum_frames(self, frames):
        """The frames of a batch of `frames` frames whose psd and dB rows are read back (trace): first, last, around a
        cumulation boundary, a few inside."""
        return sorted({0, min(1, frames - 1), frames - 1, frames // 2, min(99, frames - 1), min(100, frames - 1), frames // 3})

    def run_oracle(self):
        """One oracle receiver per band, attached and detached at the bank's frames, bands on threads of their own."""
        if hasattr(self, "outs"):
            return

        def band_events(b):
            ev, pos = [], 0  # (frame, "attach", bin) / (frame, "detach", lid), in the bank's call order
            for s in self.steps:
                if s[0] == "attach" and s[1] == b:
                    ev.append((pos, "attach", s[2]))
                elif s[0] == "detach" and s[1] == b:
                    ev.append((pos, "detach", s[2]))
                elif s[0] == "set" and s[2] in (None, b) and not _refused(s):
                    ev.append((pos, "set", (s[1], s[3])))
                elif s[0] == "defer":
                    ev += [(at, "attach", bn) for band, bn, at in s[2] if band == b]
                    # (controls called while the listen half is pending: behind the batch's last frame, behind its attaches)
                    ev += [(pos + s[1], "set", (t[1], t[3])) for t in (s[3] if len(s) > 3 else [])
                           if t[2] in (None, b) and t[1] != "signal_debounce" and not _refused(t)]
                if s[0] in ("batch", "defer"):
                    pos += s[1]
            return sorted(ev, key=lambda x: x[0])  # (stable: the call order within a frame)

        def run(b):
            r = orc.Receiver(self.rate, self.n, self.edge, self.threshold[b], self.debounce, center_frequency=self.centers[b])
            for bn in self.init_bins[b]:
                r.attach(int(bn))
            L = len(self.bins[b])
            st = {"frames": [], "deb": np.zeros((self.total, L), np.uint8), "raw": np.zeros((self.total, L), np.uint8),
                  "values": np.zeros((self.total, L), np.float32), "peaks": [], "peak_frames": [], "cumulation": [],
                  # (frame, name, value, every listener's debouncer (threshold, effective, last raw, count) before the call)
                  "sets": []}
            pos = 0
            for at, kind, arg in band_events(b) + [(self.total, None, None)]:
                if at > pos:
                    out = r.process(self.frames(b, pos, at), max_peaks=max(4096, self.max_peaks))
                    st["frames"].append(out["frames"])
                    for f in ("deb", "raw", "values"):
                        st[f][pos:at, :out[f].shape[1]] = out[f]
                    st["peaks"] += out["peaks"]
                    st["peak_frames"] += [pos + int(f) for f in out["peak_frames"]]
                    st["cumulation"] += list(out["cumulation"])
                    pos = at
                if kind == "attach":
                    r.attach(int(arg))
                elif kind == "detach":
                    r.detach(int(arg))
                elif kind == "set":
                    st["sets"].append((at, arg[0], arg[1], [r.debouncer_state(l) for l in range(r.n_listeners)]))
                    getattr(r, "set_" + arg[0])(arg[1])
            st["frames"] = np.concatenate(st["frames"])
            st["peak_frames"] = np.array(st["peak_frames"], np.int64)
            return r, st

        with ThreadPoolExecutor(max(1, min(self.n_bands, 16))) as ex:
            res = list(ex.map(run, range(self.n_bands)))
        self.refs = [r for r, _ in res]
        self.outs = [o for _, o in res]
        if self.timed:  # (text, 12-value state, the frame that wrote each rune) of every listener, ticked from its first frame on
            def timed(b, lid):
                start = self.life[b][lid][0]
                text, state, at = decode(self.outs[b]["deb"][start:, lid], self.rate, self.step, [f - start for f in self.stops.get((b, lid), ())])
                return text, state, at + start
            self.decs = [[timed(b, lid) for lid in range(out["deb"].shape[1])] for b, out in enumerate(self.outs)]

    def oracle_counts(self):
        """(edges, peaks) the oracle sees over the run: a row with none of either proves nothing."""
        self.run_oracle()
        edges = sum(int(np.count_nonzero(np.diff(np.concatenate([[0], out["deb"][:, lid].astype(np.int8)])))) for out in self.outs
                    for lid in range(out["deb"].shape[1]))
        return edges, sum(len(p) for out in self.outs for p in out["peaks"])

    def live(self, b, a, e):
        """Listeners of band b that listen during [a, e) and are not detached at its end."""
        return [lid for lid, (s, d) in enumerate(self.life[b]) if s < e and (d is None or d >= e)]

    def new_bank(self, capi, stream=None):
        """stream: the bank's own (graph capture needs one); None: the current stream, which orders the input for it."""
        import torch

        bank = capi.Bank(self.rate, self.n, n_bands=self.n_bands, edge_width=self.edge, max_batch_frames=self.max_frames,
                         max_listeners=self.max_listeners, max_peaks=self.max_peaks, signal_debounce=self.debounce, trace=self.trace,
                         hop=self.hop)
        assert bank.hop == self.step, f"the bank's hop is {bank.hop}, not {self.step}"
        bank.set_stream((stream or torch.cuda.current_stream()).cuda_stream)
        if self.first_frame:
            bank.set_first_frame(self.first_frame)
        assert bank.total_frames == self.first_frame, f"a new bank at frame {bank.total_frames}, not {self.first_frame}"
        for b in range(self.n_bands):
            bank.set_center_frequency(b, self.centers[b])
            if self.threshold[b] != 15.0:
                bank.set_peak_threshold(b, self.threshold[b])
            for i, bn in enumerate(self.init_bins[b]):
                assert bank.attach(b, int(bn)) == i, f"band {b}: listener {i} got another id"
        bank.enable_results(True)
        self.begin()
        return bank

    def begin(self):
        """What check_polled collects, emptied: new_bank calls it; so does a test that feeds the stream to something else
        (a group) and holds its deliveries to check_polled."""
        self.text = [["" for _ in bins] for bins in self.bins]
        self.rune_at = [[[] for _ in bins] for bins in self.bins]
        self.edges = self.peaks = 0
        self.window = None  # (a bank that never had a window is never told about one)
        self.controls = {"edge_width": self.edge, "find_peaks": True}

    def set_window(self, bank, k):
        """Batch k's window, if it is not the one the bank has."""
        if self.windows[k] is not self.window:
            self.window = self.windows[k]
            bank.set_window(self.window)

    def apply_set(self, capi, bank, s, last, pending=False):
        """One ("set", ...) step on the bank.  last: (a, e, k) of the batch just enqueued, or None; pending: its listen
        half is pending.  self.controls follows the two controls a captured graph has baked in."""
        _, name, band, value = s
        call = {"peak_threshold": lambda v: bank.set_peak_threshold(band, v), "edge_width": bank.set_edge_width,
                "signal_debounce": lambda v: bank.set_signal_debounce(band, v), "find_peaks": bank.set_find_peaks}[name]
        refuse = capi.ERR_BAD_ARG if _refused(s) else capi.ERR_STATE if pending and name == "signal_debounce" else None
        if refuse is not None:
            try:
                call(value[1] if _refused(s) else value)
            except capi.SdrError as err:
                assert err.code == refuse, f"{s}: refused with {err.code}, not {refuse}"
                return
            raise AssertionError(f"{s}: accepted, SDR_ERR {refuse} expected")
        call(value)
        if name in self.controls:
            self.controls[name] = value
        if name == "edge_width" and last is not None:
            # the batch before ran with the width before: its records are still the oracle's, its variance included, and
            # the read's own comparison with the literal FindNoiseFloor (an error if it fails) uses that width too
            a, e, k = last
            for b in range(self.n_bands):
                recs = bank.read_frame_records(b)
                same = nan_equal_bits if self.nan_ok else bits_equal
                for f in REC_FIELDS:
                    assert same(recs[f], self.outs[b]["frames"][f][a:e].copy()), f"band {b} batch {k} field {f}, read behind {s}"

    def gone(self, a):
        """(band, listener) pairs detached before frame a whose slot nobody has taken over by then."""
        return [(b, lid) for b in range(self.n_bands) for lid, (_, d) in enumerate(self.life[b])
                if d is not None and d <= a and (self.heir[b][lid] is None or self.life[b][self.heir[b][lid]][0] > a)]

    def check_polled(self, res, a, e):
        """One delivered batch against the stitched oracle stream, for the listeners live in it; detached ones deliver nothing."""
        ne, npk = check_batch_polled(res, self.outs, a, e, None, self.text, self.n_bands,
                                     live=[self.live(b, a, e) for b in range(self.n_bands)], gone=self.gone(a), rune_at=self.rune_at,
                                     max_peaks=self.max_peaks, first_frame=self.first_frame, slot=self.slot)
        self.edges += ne
        self.peaks += npk

    def check_device(self, bank, a, e, k, cumulations=True):
        """What the last batch left on the device: frame records, keying bits, cumulation rows; with trace, the tap."""
        check_device_batch(bank, self.outs, a, e, self.n_bands, [self.live(b, a, e) for b in range(self.n_bands)], k, cumulations,
                           same=nan_equal_bits if self.nan_ok else None, max_peaks=self.max_peaks, slot=self.slot)
        if self.trace:
            self.check_trace(bank, a, e, k)

    def check_trace(self, bank, a, e, k):
        """The tap of the last batch: the value handed to Listen, raw and debounced state of every listener, frame by frame;
        psd and dB spectrum of the sampled frames."""
        same = nan_equal_bits if self.nan_ok else bits_equal
        for b in range(self.n_bands):
            out = self.outs[b]
            for lid in self.live(b, a, e):
                v, raw, deb = bank.read_trace(b, self.slot[b][lid])
                s = max(self.life[b][lid][0] - a, 0)  # (a listener bound inside the batch: nothing was handed to it before)
                assert same(v[s:], out["values"][a + s:e, lid].copy()), f"band {b} listener {lid} batch {k} tap values"
                assert np.array_equal(raw[s:], out["raw"][a + s:e, lid]), f"band {b} listener {lid} batch {k} raw bits"
                assert np.array_equal(deb, out["deb"][a:e, lid]), f"band {b} listener {lid} batch {k} debounced bits"
            for f in self.spectrum_frames(e - a):
                sp, psd = bank.read_spectrum(b, f)
                want_sp, want_psd = orc.iq_to_spectrum_and_psd(self.frames(b, a + f, a + f + 1))
                assert same(psd, want_psd), f"band {b} batch {k} frame {a + f} psd"
                assert same(sp, want_sp), f"band {b} batch {k} frame {a + f} spectrum"

    def check_end(self, bank, min_edges, activity=True):
        for b in range(self.n_bands):
            for lid in range(len(self.bins[b])):
                text, state = self.decs[b][lid][:2] if self.timed else (self.refs[b].text(lid), self.refs[b].decoder_state(lid))
                assert self.text[b][lid] == text, f"band {b} listener {lid} text"
                if self.heir[b][lid] is None:  # (else the slot holds its heir's decoder)
                    assert np.array_equal(bank.read_decoder_state(b, self.slot[b][lid]), state), f"band {b} listener {lid} state"
                if self.timed:
                    assert np.array_equal(np.array(self.rune_at[b][lid], np.int64), frames32(self.decs[b][lid][2], self.first_frame)), \
                        f"band {b} listener {lid} rune frames"
        assert bank.total_frames == self.first_frame + self.total, f"{bank.total_frames} frames after {self.total} from {self.first_frame}"
        assert bank.read_drop_counters() == (0, 0), "runes or edges dropped"
        if activity:
            n_carriers = sum(len(c) for c in self.carriers)
            assert self.edges > min_edges * n_carriers and self.peaks > 0 and any(len(t) > 0 for row in self.text for t in row), \
                f"{self.edges} edges, {self.peaks} peaks: the run shows too little"

    # -- input -------------------------------------------------------------------------------------------------------------
    def _device_input(self):
        """The whole stream of every band in device memory, [band][sample][2] (float32 or int16 by the path), `pad` samples
        of zeros behind each."""
        import torch

        if not hasattr(self, "_dev"):
            src = self.q if self.path in SC16_PATHS or self.path in IQ8_PATHS else self.stream
            host = np.zeros((self.n_bands, src[0].shape[0] + self.pad, 2), src[0].dtype)
            for b in range(self.n_bands):
                host[b, :src[b].shape[0]] = src[b]
            self._dev = torch.from_numpy(host).cuda()
        return self._dev

    def device_batch(self, a, e):
        """Dense frames [a, e) of every band in device memory, [band][frame][2N]."""
        return self._device_input()[:, a * self.n:e * self.n].contiguous()

    def _enqueue(self, bank, a, e):
        """One batch [a, e) through the case's input path (not the graph paths); returns what must outlive the call."""
        sc16 = self.path in SC16_PATHS
        if self.path.startswith("device") and self.hop:
            dev = self._device_input()
            ptr = dev.data_ptr() + a * self.hop * 2 * dev.element_size()
            if self.path in IQ8_PATHS:
                bank.process_device_stream_iq8(ptr, e - a, dev.shape[1], IQ8_PATHS[self.path])
            else:
                (bank.process_device_stream_sc16 if sc16 else bank.process_device_stream)(ptr, e - a, dev.shape[1])
            return dev
        if self.path.startswith("device"):
            batch = self.device_batch(a, e)
            if self.path in IQ8_PATHS:
                bank.process_device_iq8(batch.data_ptr(), e - a, IQ8_PATHS[self.path])
            else:
                (bank.process_device_sc16 if sc16 else bank.process_device)(batch.data_ptr(), e - a)
            return batch
        lo, hi = (a - 1) * self.step + self.n if a else 0, (e - 1) * self.step + self.n  # the samples the batch adds
        for b in range(self.n_bands):
            if self.path == "staged":
                assert bank.push_iq(b, self.rate, self.stream[b][lo:hi].reshape(-1)) == 0, f"band {b}: push refused"
            elif self.path == "staged_sc16":
                assert bank.push_iq_sc16(b, self.rate, self.q[b][lo:hi].reshape(-1)) == 0, f"band {b}: push refused"
            elif self.path in IQ8_PATHS:
                assert bank.push_iq8(b, self.rate, self.q[b][lo:hi].reshape(-1), IQ8_PATHS[self.path]) == 0, f"band {b}: push refused"
            else:  # KiwiSDR: the batch's frames in messages of up to 1, 2, 5, 12 ... frames, as the websocket delivers them
                f, sizes, n = a, (1, 2, 5, 12, 40), self.n
                while f < e:
                    k = min(sizes[(f - a) % len(sizes)], e - f)
                    assert bank.push_kiwi_snd(b, self.rate, KIWI_HEADER + self.q[b][f * n:(f + k) * n].astype(">i2").tobytes()) == 0, \
                        f"band {b}: message refused"
                    f += k
        got = bank.process_staged()
        assert got == e - a, f"{got} staged frames, not {e - a}"
        return None

    # -- runs --------------------------------------------------------------------------------------------------------------
    def run(self, capi, min_edges=20, lag=False, activity=True, prepare=None, before_poll=None):
        """Every step on one bank, each batch checked when it is delivered.  lag: a batch is polled only once the next one
        is enqueued (the listen stream may then still run one batch while the next batch's spectral stages start), and
        what stays on the device is checked for the last batch only.  prepare(bank): called on the new bank, in front of
        the first step; before_poll(bank, k): called in front of the sdr_poll that delivers batch k (neither on the graph
        paths)."""
        if self.path.startswith("graph"):
            return self.run_graph(capi, min_edges, activity)
        self.run_oracle()
        bank = self.new_bank(capi)
        if prepare:
            prepare(bank)
        pos, k = 0, 0
        pending = []  # (first frame, end, batch index, input) enqueued and not yet polled

        def deliver(last):
            a, e, i, _ = pending.pop(0)
            if before_poll:
                before_poll(bank, i)
            res = bank.poll(wait=True)
            assert res["batch_index"] == i, f"batch {i} delivered as {res['batch_index']}"
            self.check_polled(res, a, e)
            if last:
                self.check_device(bank, a, e, i)
        slots = [len(bins) for bins in self.init_bins]  # the next listener of each band, in the oracle's numbering
        for s in self.steps:
            if s[0] == "attach":
                got = bank.attach(s[1], int(s[2]))
                assert got == self.slot[s[1]][slots[s[1]]], f"band {s[1]}: attach gave listener {got}"
                slots[s[1]] += 1
                continue
            if s[0] == "detach":
                bank.detach(s[1], self.slot[s[1]][s[2]])
                continue
            if s[0] == "stop":
                bank.listener_stop(s[1], self.slot[s[1]][s[2]])
                continue
            if s[0] == "set":
                self.apply_set(capi, bank, s, (self.spans[k - 1] + (k - 1,)) if k else None)
                continue
            a, e = pos, pos + s[1]
            self.set_window(bank, k)
            if s[0] == "defer":
                bank.defer_listen(True)
                batch = self._enqueue(bank, a, e)
                pk = bank.poll_peaks(wait=True)
                assert pk["first_frame"] == self.first_frame + a, f"batch {k}: peaks of frame {pk['first_frame']}"
                for band, bn, at in s[2]:
                    got = bank.attach_at(band, int(bn), self.first_frame + at)
                    assert got == self.slot[band][slots[band]], f"band {band}: attach_at gave listener {got}"
                    slots[band] += 1
                for t in s[3] if len(s) > 3 else []:
                    self.apply_set(capi, bank, t, (a, e, k), pending=True)
                bank.process_listen()
                bank.defer_listen(False)
            else:
                batch = self._enqueue(bank, a, e)
            pending.append((a, e, k, batch))
            if len(pending) > lag:
                deliver(not lag)
            pos, k = e, k + 1
        while pending:
            deliver(len(pending) == 1)
        self.check_end(bank, min_edges, activity)
        return bank

    def run_graph(self, capi, min_edges=20, activity=True):
        """The graph paths: replays of sdr_graph_batches() batches of one length, a release and a new capture after every
        listener change and before a replay with another window.  Each delivered batch is checked; what stays on the
        device after the last batch of every replay."""
        import torch

        assert all(s[0] in ("batch", "attach", "detach", "set") for s in self.steps), "graph mode takes no deferred batch"
        per = {s[1] for s in self.steps if s[0] == "batch"}
        assert len(per) == 1, "graph mode: batches of one length"
        per = per.pop()
        self.run_oracle()
        bank = self.new_bank(capi, torch.cuda.Stream())
        K = bank.graph_batches
        sc16, iq8 = self.path == "graph_sc16", IQ8_PATHS.get(self.path)
        slots = [len(bins) for bins in self.init_bins]
        pos, k, captured, run, baked = 0, 0, False, [], None  # baked: self.controls as of the capture
        for s in self.steps + [("end",)]:
            if s[0] == "batch":
                run.append((pos, pos + per))
                pos += per
                if len(run) < K:
                    continue
                assert all(w is self.windows[k] for w in self.windows[k:k + K]), "graph mode: one window per replay"
                if captured and self.windows[k] is not self.window:
                    bank.graph_release()
                    captured = False
                self.set_window(bank, k)
                batches = [self.device_batch(a, e) for a, e in run]
                torch.cuda.synchronize()  # (the input is written on torch's stream, the bank reads it on its own)

                def launch():
                    ptrs = [x.data_ptr() for x in batches]
                    if iq8 is not None:
                        bank.graph_launch_iq8(ptrs, iq8)
                    else:
                        (bank.graph_launch_sc16 if sc16 else bank.graph_launch)(ptrs)
                if captured and baked != self.controls:  # a control the capture has baked in changed: the replay is refused, nothing has run
                    try:
                        launch()
                    except capi.SdrError as err:
                        assert err.code == capi.ERR_STATE, f"replay behind a changed control: refused with {err.code}"
                    else:
                        raise AssertionError("a replay behind a changed edge width or find_peaks was accepted")
                    assert bank.total_frames == self.first_frame + run[0][0], "a refused replay moved the bank"
                    bank.graph_release()
                    captured = False
                if not captured:
                    if iq8 is not None:
                        bank.graph_capture_iq8(per, iq8)
                    else:
                        (bank.graph_capture_sc16 if sc16 else bank.graph_capture)(per)
                    captured, baked = True, dict(self.controls)
                launch()
                for a, e in run:
                    res = bank.poll(wait=True)
                    assert res["batch_index"] == k, f"batch {k} delivered as {res['batch_index']}"
                    self.check_polled(res, a, e)
                    k += 1
                bank.sync()
                assert bank.total_frames == self.first_frame + pos, f"{bank.total_frames} frames after {pos} from {self.first_frame}"
                self.check_device(bank, run[-1][0], run[-1][1], k - 1, cumulations=False)
                run = []
                continue
            assert not run, "graph mode: listener changes only between replays"
            if s[0] == "end":
                break
            if s[0] == "set":  # (with the capture in place)
                self.apply_set(capi, bank, s, (self.spans[k - 1] + (k - 1,)) if k else None)
                continue
            if captured:  # a listener change invalidates the capture (capi_graph.hip): release, capture again later
                bank.graph_release()
                captured = False
            if s[0] == "attach":
                got = bank.attach(s[1], int(s[2]))
                assert got == self.slot[s[1]][slots[s[1]]], f"band {s[1]}: attach gave listener {got}"
                slots[s[1]] += 1
            else:
                bank.detach(s[1], self.slot[s[1]][s[2]])
        self.check_end(bank, min_edges, activity)
        return bank
