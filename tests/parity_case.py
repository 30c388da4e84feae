"""One bank's stream against the CPU oracle, bit for bit: the `Case` driver that test_listener_band_geometry.py and
test_gpu_fuzz_paths.py share (a plain helper module, not a test file).

A Case holds n_bands bands of keyed carriers and a list of steps; it runs one oracle receiver per band, attached and
detached at the bank's frames and stitched into one stream per band (a listener's keying column is zero before it is
attached), and compares with what sdr_poll delivers and what stays on the device: frame records, keying bits, edges,
runes, decoder state, the exact cumulation rows (and the kept row: never below the exact one, equal at and beside every
peak), peaks with their frequencies, and drop counters of 0.

The input reaches the bank by one of the paths of include/sdrainer_hip.h:
  "device"       float32 in device memory (sdr_process_device)
  "device_sc16"  complex int16 in device memory (sdr_process_device_sc16)
  "staged"       float32 from the host (sdr_push_iq -> sdr_process_staged)
  "staged_sc16"  complex int16 from the host (sdr_push_iq_sc16)
  "kiwi"         KiwiSDR SND payloads, big-endian int16 (sdr_push_kiwi_snd), a batch's frames in several messages
  "graph"        hipGraph replays of float32 batches (sdr_graph_capture / sdr_graph_launch)
  "graph_sc16"   the same for sc16 (sdr_graph_capture_sc16 / sdr_graph_launch_sc16)
The oracle always reads the float32 values the bank was given: for sc16 and KiwiSDR input float32(x) / 32767.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import oracle as orc
from sdrainer_amd import synth
from test_gpu_parity_bench_sizes import _check_batch_polled, _check_device_batch

RATE = 2_000_000
PATHS = ("device", "device_sc16", "staged", "staged_sc16", "kiwi", "graph", "graph_sc16")
SC16_PATHS = ("device_sc16", "staged_sc16", "kiwi", "graph_sc16")
KIWI_HEADER = bytes([0x01] + [7] * 16)  # the 17 bytes in front of an SND message's samples (flags, sequence, smeter)


def nan_equal_bits(a, b):
    """Bit for bit, except that two NaNs are equal whatever their sign and payload (which are not part of the contract)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return np.array_equal(np.where(both_nan, 0, a.view(u)), np.where(both_nan, 0, b.view(u)))


def sc16_to_float32(q):
    """The float32 values an sc16 sample stands for (include/sdrainer_hip.h: float32(x) / 32767, one rounding)."""
    return np.asarray(q, np.int16).astype(np.float32) / np.float32(32767.0)


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


class Case:
    """One bank's stream: bands of keyed carriers, the listeners attached before the first frame, then a list of steps
       ("batch", frames)                      an eager batch
       ("defer", frames, [(band, bin, s)])    a deferred batch; after its peaks, sdr_attach_at(band, bin, s) in order
       ("attach", band, bin) / ("detach", band, lid)   between batches
    (steps may also be a function of the carriers' bins per band, which exist once the input does)

    Per band (a value, or a list with one per band): peak threshold and centre frequency.  The sample rate, the edge width
    and the debounce are the bank's (sdr_config), one for all of its bands: sdr_set_signal_debounce reaches only the
    listeners attached at the time, as the reference's Receiver.SetSignalDebounce does, and every later listener starts
    from the bank's value.  `bands` replaces the synthetic carriers: one
    (float32 [total, 2N] host array, int16 [total, 2N] or None, carrier bins) per band - the int16 array is what the sc16
    and KiwiSDR paths send, and the float32 one must then be its value (sc16_to_float32).  Graph paths take batches of one
    length, sdr_graph_batches() of them per replay, with attach / detach only between replays (each one is followed by a
    release and a new capture); no deferred batches.  nan_ok: the oracle's stream holds NaN (a silent run: -Inf and then
    NaN in the rolling means and thresholds), and NaN compares by class in the float fields."""

    def __init__(self, n, n_bands, carriers, listeners, steps, seed, rate=RATE, free_last=True, max_listeners=None, total_frames=None,
                 *, edge=None, debounce=1, threshold=15.0, centers=None, path="device", bands=None, init_bins=None, max_peaks=1024,
                 nan_ok=False):
        assert path in PATHS, path
        self.n, self.n_bands, self.rate, self.path, self.nan_ok = n, n_bands, rate, path, nan_ok
        self.edge = synth.default_edge_width(n) if edge is None else edge
        self.debounce, self.threshold = debounce, _per_band(threshold, n_bands)
        self.total = total_frames or sum(s[1] for s in steps if s[0] in ("batch", "defer"))
        self.centers = [14000000 + 100000 * b for b in range(n_bands)] if centers is None else _per_band(centers, n_bands)
        self.max_peaks = max_peaks
        self.dev_iq, self.host_iq, self.q, self.carriers, self.init_bins = [], [], [], [], []
        for b in range(n_bands):
            if bands is None:
                iq, bins, _ = synth.make_band_torch(self.total, rate, n, carriers, seed=seed + 17 * b, device="cuda", free_last_window=free_last)
                self.dev_iq.append(iq)
                self.q.append(None)
            else:
                f32, q, bins = bands[b]
                assert f32.shape == (self.total, 2 * n) and f32.dtype == np.float32
                if path in SC16_PATHS:
                    assert q is not None and np.array_equal(sc16_to_float32(q).view(np.uint32), f32.view(np.uint32))
                self.host_iq.append(f32)
                self.q.append(q)
            self.carriers.append([int(x) for x in bins])
            if init_bins is not None:
                self.init_bins.append([int(x) for x in init_bins[b]])
            else:
                self.init_bins.append((self.carriers[b] + _extra_bins(n, bins, max(0, listeners - len(bins)), seed + 17 * b))[:listeners])
        self.steps = steps = steps(self.carriers) if callable(steps) else steps
        assert self.total == sum(s[1] for s in steps if s[0] in ("batch", "defer"))
        self.max_frames = max(s[1] for s in steps if s[0] in ("batch", "defer"))
        late = sum(1 for s in steps if s[0] == "attach") + sum(len(s[2]) for s in steps if s[0] == "defer")
        self.max_listeners = max_listeners or max(1, max(len(b) for b in self.init_bins) + late)
        # every listener of every band: (attached at frame, detached at frame or None)
        self.life = [[(0, None) for _ in bins] for bins in self.init_bins]
        self.bins = [list(bins) for bins in self.init_bins]
        pos = 0
        for s in steps:
            if s[0] == "attach":
                self.bins[s[1]].append(s[2])
                self.life[s[1]].append((pos, None))
            elif s[0] == "detach":
                self.life[s[1]][s[2]] = (self.life[s[1]][s[2]][0], pos)
            else:
                for band, bn, at in s[2] if s[0] == "defer" else []:
                    assert pos <= at < pos + s[1]
                    self.bins[band].append(bn)
                    self.life[band].append((at, None))
                pos += s[1]

    def oracle_input(self, b):
        """The float32 values band b is given, host side."""
        return self.host_iq[b] if self.host_iq else self.dev_iq[b].cpu().numpy()

    def run_oracle(self):
        """One oracle receiver per band, attached and detached at the bank's frames, bands on threads of their own."""
        def band_events(b):
            ev, pos = [], 0  # (frame, "attach", bin) / (frame, "detach", lid), in the bank's call order
            for s in self.steps:
                if s[0] == "attach" and s[1] == b:
                    ev.append((pos, "attach", s[2]))
                elif s[0] == "detach" and s[1] == b:
                    ev.append((pos, "detach", s[2]))
                elif s[0] == "defer":
                    ev += [(at, "attach", bn) for band, bn, at in s[2] if band == b]
                if s[0] in ("batch", "defer"):
                    pos += s[1]
            return ev

        def run(b):
            host = self.oracle_input(b)
            r = orc.Receiver(self.rate, self.n, self.edge, self.threshold[b], self.debounce, center_frequency=self.centers[b])
            for bn in self.init_bins[b]:
                r.attach(int(bn))
            L = len(self.bins[b])
            st = {"frames": [], "deb": np.zeros((self.total, L), np.uint8), "peaks": [], "peak_frames": [], "cumulation": []}
            pos = 0
            for at, kind, arg in band_events(b) + [(self.total, None, None)]:
                if at > pos:
                    out = r.process(host[pos:at], max_peaks=max(4096, self.max_peaks))
                    st["frames"].append(out["frames"])
                    st["deb"][pos:at, :out["deb"].shape[1]] = out["deb"]
                    st["peaks"] += out["peaks"]
                    st["peak_frames"] += [pos + int(f) for f in out["peak_frames"]]
                    st["cumulation"] += list(out["cumulation"])
                    pos = at
                if kind == "attach":
                    r.attach(int(arg))
                elif kind == "detach":
                    r.detach(int(arg))
            st["frames"] = np.concatenate(st["frames"])
            st["peak_frames"] = np.array(st["peak_frames"], np.int64)
            return r, st

        with ThreadPoolExecutor(max(1, min(self.n_bands, 16))) as ex:
            res = list(ex.map(run, range(self.n_bands)))
        self.refs = [r for r, _ in res]
        self.outs = [o for _, o in res]

    def live(self, b, a, e):
        """Listeners of band b that listen during [a, e) and are not detached at its end."""
        return [lid for lid, (s, d) in enumerate(self.life[b]) if s < e and (d is None or d >= e)]

    def new_bank(self, capi, stream=None):
        """stream: the bank's own (graph capture needs one); None: the current stream, which orders the input for it."""
        import torch

        bank = capi.Bank(self.rate, self.n, n_bands=self.n_bands, edge_width=self.edge, max_batch_frames=self.max_frames,
                         max_listeners=self.max_listeners, max_peaks=self.max_peaks, signal_debounce=self.debounce)
        bank.set_stream((stream or torch.cuda.current_stream()).cuda_stream)
        for b in range(self.n_bands):
            bank.set_center_frequency(b, self.centers[b])
            if self.threshold[b] != 15.0:
                bank.set_peak_threshold(b, self.threshold[b])
            for i, bn in enumerate(self.init_bins[b]):
                assert bank.attach(b, int(bn)) == i
        bank.enable_results(True)
        self.text = [["" for _ in bins] for bins in self.bins]
        self.edges = self.peaks = 0
        return bank

    def gone(self, a):
        """(band, listener) pairs detached before frame a."""
        return [(b, lid) for b in range(self.n_bands) for lid, (_, d) in enumerate(self.life[b]) if d is not None and d <= a]

    def check_polled(self, res, a, e):
        """One delivered batch against the stitched oracle stream, for the listeners live in it; detached ones deliver nothing."""
        ne, npk = _check_batch_polled(res, self.outs, a, e, None, self.text, self.n_bands,
                                      live=[self.live(b, a, e) for b in range(self.n_bands)], gone=self.gone(a))
        self.edges += ne
        self.peaks += npk

    def check_device(self, bank, a, e, k, cumulations=True):
        """What the last batch left on the device: frame records, keying bits, cumulation rows."""
        _check_device_batch(bank, self.outs, a, e, self.n_bands, [self.live(b, a, e) for b in range(self.n_bands)], k, cumulations,
                            same=nan_equal_bits if self.nan_ok else None)

    def check_end(self, bank, min_edges, activity=True):
        for b in range(self.n_bands):
            for lid in range(len(self.bins[b])):
                assert self.text[b][lid] == self.refs[b].text(lid), f"band {b} listener {lid} text"
                assert np.array_equal(bank.read_decoder_state(b, lid), self.refs[b].decoder_state(lid)), f"band {b} listener {lid} state"
        assert bank.read_drop_counters() == (0, 0)
        if activity:
            n_carriers = sum(len(c) for c in self.carriers)
            assert self.edges > min_edges * n_carriers and self.peaks > 0 and any(len(t) > 0 for row in self.text for t in row)

    # -- input -------------------------------------------------------------------------------------------------------------
    def _device_input(self):
        """The whole stream of every band in device memory, [band][frame][2N] per band (float32 or int16 by the path)."""
        import torch

        if self.dev_iq:
            return self.dev_iq
        if not hasattr(self, "_dev"):
            src = self.q if self.path in SC16_PATHS else self.host_iq
            self._dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in src]
        return self._dev

    def _device_batch(self, a, e):
        import torch

        return torch.stack([iq[a:e] for iq in self._device_input()]).contiguous()

    def _enqueue(self, bank, a, e):
        """One batch [a, e) through the case's input path (not the graph paths); returns what must outlive the call."""
        if self.path in ("device", "device_sc16"):
            batch = self._device_batch(a, e)
            (bank.process_device_sc16 if self.path == "device_sc16" else bank.process_device)(batch.data_ptr(), e - a)
            return batch
        for b in range(self.n_bands):
            if self.path == "staged":
                assert bank.push_iq(b, self.rate, self.host_iq[b][a:e].reshape(-1)) == 0
            elif self.path == "staged_sc16":
                assert bank.push_iq_sc16(b, self.rate, self.q[b][a:e].reshape(-1)) == 0
            else:  # KiwiSDR: the batch's frames in messages of up to 1, 2, 5, 12 ... frames, as the websocket delivers them
                f, sizes = a, (1, 2, 5, 12, 40)
                while f < e:
                    k = min(sizes[(f - a) % len(sizes)], e - f)
                    assert bank.push_kiwi_snd(b, self.rate, KIWI_HEADER + self.q[b][f:f + k].astype(">i2").tobytes()) == 0
                    f += k
        assert bank.process_staged() == e - a
        return None

    # -- runs --------------------------------------------------------------------------------------------------------------
    def run(self, capi, min_edges=20, lag=False, activity=True):
        """Every step on one bank, each batch checked when it is delivered.  lag: a batch is polled only once the next one
        is enqueued (the listen stream may then still run one batch while the next batch's spectral stages start), and
        what stays on the device is checked for the last batch only."""
        if self.path.startswith("graph"):
            return self.run_graph(capi, min_edges, activity)
        self.run_oracle()
        bank = self.new_bank(capi)
        pos, k = 0, 0
        pending = []  # (first frame, end, batch index, input) enqueued and not yet polled

        def deliver(last):
            a, e, i, _ = pending.pop(0)
            res = bank.poll(wait=True)
            assert res["batch_index"] == i
            self.check_polled(res, a, e)
            if last:
                self.check_device(bank, a, e, i)
        slots = [len(bins) for bins in self.init_bins]  # (no attach follows a detach on a band: ids are the oracle's)
        for s in self.steps:
            if s[0] == "attach":
                assert bank.attach(s[1], int(s[2])) == slots[s[1]]
                slots[s[1]] += 1
                continue
            if s[0] == "detach":
                bank.detach(s[1], s[2])
                continue
            a, e = pos, pos + s[1]
            if s[0] == "defer":
                bank.defer_listen(True)
                batch = self._enqueue(bank, a, e)
                pk = bank.poll_peaks(wait=True)
                assert pk["first_frame"] == a
                for band, bn, at in s[2]:
                    assert bank.attach_at(band, int(bn), at) == slots[band]
                    slots[band] += 1
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
        listener change.  Each delivered batch is checked; what stays on the device after the last batch of every replay."""
        import torch

        assert all(s[0] in ("batch", "attach", "detach") for s in self.steps), "graph mode takes no deferred batch"
        per = {s[1] for s in self.steps if s[0] == "batch"}
        assert len(per) == 1, "graph mode: batches of one length"
        per = per.pop()
        self.run_oracle()
        bank = self.new_bank(capi, torch.cuda.Stream())
        K = bank.graph_batches
        sc16 = self.path == "graph_sc16"
        slots = [len(bins) for bins in self.init_bins]
        pos, k, captured, run = 0, 0, False, []
        for s in self.steps + [("end",)]:
            if s[0] == "batch":
                run.append((pos, pos + per))
                pos += per
                if len(run) < K:
                    continue
                if not captured:
                    (bank.graph_capture_sc16 if sc16 else bank.graph_capture)(per)
                    captured = True
                batches = [self._device_batch(a, e) for a, e in run]
                torch.cuda.synchronize()  # (the input is written on torch's stream, the bank reads it on its own)
                (bank.graph_launch_sc16 if sc16 else bank.graph_launch)([x.data_ptr() for x in batches])
                for a, e in run:
                    res = bank.poll(wait=True)
                    assert res["batch_index"] == k
                    self.check_polled(res, a, e)
                    k += 1
                bank.sync()
                assert bank.total_frames == pos
                self.check_device(bank, run[-1][0], run[-1][1], k - 1, cumulations=False)
                run = []
                continue
            assert not run, "graph mode: listener changes only between replays"
            if s[0] == "end":
                break
            if captured:  # a listener change invalidates the capture (capi_graph.hip): release, capture again later
                bank.graph_release()
                captured = False
            if s[0] == "attach":
                assert bank.attach(s[1], int(s[2])) == slots[s[1]]
                slots[s[1]] += 1
            else:
                bank.detach(s[1], s[2])
        self.check_end(bank, min_edges, activity)
        return bank
