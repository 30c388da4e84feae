"""The HIP path against the CPU oracle, bit for bit, at the listener and band counts where the hot path switches code:

  512 / 513 slots at N = 16384   k_fft_r32 (and its wide tap, read by k_cum_refine) or the 16-point k_fft_psd<14>
  4096 / 4097 listeners          the one-frame FFT kernel's LDS tap or its drain path
  many gather rows               k_listen_gather's grid.y = ceil(n_slots / 64), decoder groups of 16
  many bands                     grid.y = n_bands in the FFT kernels, k_fft_r32's per-band claim counters, 64 bands of
                                 config 5 on one GPU (eager and as graph replays)
  the small plan                 B * N <= 8192: the gather on the peaks stream, behind many sdr_attach_at slot writes

and across the transitions between them inside one stream: the slot pool is a high-water mark, so the 513th listener
moves a bank off k_fft_r32 for good, with cumulation and decoder state carried over, and a listener bound with
sdr_attach_at inside a deferred batch can make that move between the batch's FFT and its listen half.

Listeners beyond the keyed carriers sit on bins 0 and N - 1 (the wide tap's wrap-around neighbours), beside carriers
(the wide tap stores bin - 1 and bin + 1), on a carrier a second time and on noise bins.  The oracle runs every band
segment by segment, with each attach and detach at the frame where the bank applies it; its outputs are stitched into
one stream per band (a listener's keying column is zero before it is attached) and compared with what sdr_poll
delivers and what stays on the device: frame records, keying bits, edges, runes, decoder state, the exact cumulation
rows (and the kept row: never below the exact one, equal at and beside every peak) and peaks.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle as orc
from sdrainer_amd import synth
from test_gpu_parity_bench_sizes import _check_batch_polled, _check_device_batch

pytestmark = pytest.mark.gpu

RATE = 2_000_000


@pytest.fixture(scope="module")
def capi():
    from sdrainer_amd import capi as c
    c.load()
    return c


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


class Case:
    """One bank's stream: bands of keyed carriers, the listeners attached before the first frame, then a list of steps
       ("batch", frames)                      an eager batch
       ("defer", frames, [(band, bin, s)])    a deferred batch; after its peaks, sdr_attach_at(band, bin, s) in order
       ("attach", band, bin) / ("detach", band, lid)   between batches
    (steps may also be a function of the carriers' bins per band, which exist once the input does)
    """

    def __init__(self, n, n_bands, carriers, listeners, steps, seed, rate=RATE, free_last=True, max_listeners=None, total_frames=None):
        self.n, self.n_bands, self.rate = n, n_bands, rate
        self.edge = synth.default_edge_width(n)
        self.total = total_frames or sum(s[1] for s in steps if s[0] in ("batch", "defer"))
        self.centers = [14000000 + 100000 * b for b in range(n_bands)]
        self.dev_iq, self.carriers, self.init_bins = [], [], []
        for b in range(n_bands):
            iq, bins, _ = synth.make_band_torch(self.total, rate, n, carriers, seed=seed + 17 * b, device="cuda", free_last_window=free_last)
            self.dev_iq.append(iq)
            self.carriers.append([int(x) for x in bins])
            self.init_bins.append((self.carriers[b] + _extra_bins(n, bins, max(0, listeners - carriers), seed + 17 * b))[:listeners])
        self.steps = steps = steps(self.carriers) if callable(steps) else steps
        assert self.total == sum(s[1] for s in steps if s[0] in ("batch", "defer"))
        self.max_frames = max(s[1] for s in steps if s[0] in ("batch", "defer"))
        late = sum(1 for s in steps if s[0] == "attach") + sum(len(s[2]) for s in steps if s[0] == "defer")
        self.max_listeners = max_listeners or listeners + late
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
            host = self.dev_iq[b].cpu().numpy()
            r = orc.Receiver(self.rate, self.n, self.edge, 15.0, 1, center_frequency=self.centers[b])
            for bn in self.init_bins[b]:
                r.attach(int(bn))
            L = len(self.bins[b])
            st = {"frames": [], "deb": np.zeros((self.total, L), np.uint8), "peaks": [], "peak_frames": [], "cumulation": []}
            pos = 0
            for at, kind, arg in band_events(b) + [(self.total, None, None)]:
                if at > pos:
                    out = r.process(host[pos:at])
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
                         max_listeners=self.max_listeners, max_peaks=1024)
        bank.set_stream((stream or torch.cuda.current_stream()).cuda_stream)
        for b in range(self.n_bands):
            bank.set_center_frequency(b, self.centers[b])
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
        _check_device_batch(bank, self.outs, a, e, self.n_bands, [self.live(b, a, e) for b in range(self.n_bands)], k, cumulations)

    def check_end(self, bank, min_edges):
        for b in range(self.n_bands):
            for lid in range(len(self.bins[b])):
                assert self.text[b][lid] == self.refs[b].text(lid), f"band {b} listener {lid} text"
                assert np.array_equal(bank.read_decoder_state(b, lid), self.refs[b].decoder_state(lid)), f"band {b} listener {lid} state"
        assert bank.read_drop_counters() == (0, 0)
        n_carriers = sum(len(c) for c in self.carriers)
        assert self.edges > min_edges * n_carriers and self.peaks > 0 and any(len(t) > 0 for row in self.text for t in row)

    def run(self, capi, min_edges=20, lag=False):
        """Every step on one bank, each batch checked when it is delivered.  lag: a batch is polled only once the next one
        is enqueued (the listen stream may then still run one batch while the next batch's spectral stages start), and
        what stays on the device is checked for the last batch only."""
        import torch

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
        slots = [len(bins) for bins in self.init_bins]  # (no attach follows a detach here: ids are the oracle's)
        for s in self.steps:
            if s[0] == "attach":
                assert bank.attach(s[1], int(s[2])) == slots[s[1]]
                slots[s[1]] += 1
                continue
            if s[0] == "detach":
                bank.detach(s[1], s[2])
                continue
            a, e = pos, pos + s[1]
            batch = torch.stack([iq[a:e] for iq in self.dev_iq]).contiguous()  # [band][frame][2N]
            if s[0] == "defer":
                bank.defer_listen(True)
                bank.process_device(batch.data_ptr(), e - a)
                pk = bank.poll_peaks(wait=True)
                assert pk["first_frame"] == a
                for band, bn, at in s[2]:
                    assert bank.attach_at(band, int(bn), at) == slots[band]
                    slots[band] += 1
                bank.process_listen()
                bank.defer_listen(False)
            else:
                bank.process_device(batch.data_ptr(), e - a)
            pending.append((a, e, k, batch))
            if len(pending) > lag:
                deliver(not lag)
            pos, k = e, k + 1
        while pending:
            deliver(len(pending) == 1)
        self.check_end(bank, min_edges)
        return bank


# -- 1. N = 16384 at 512 and 513 slots -----------------------------------------------------------------------------------

@pytest.mark.parametrize("slots", [512, 513])
def test_fft_r32_slot_limit(capi, slots):
    """N = 16384, 256 keyed carriers and `slots` listeners, two 1024-frame batches (n_frames * n_bands >= 1024, so the
    frame count alone would pick k_fft_r32).  fft_choice (host/batch_plan.h, `tap_n <= kR32MaxTap`) selects k_fft_r32 at
    512 slots - register tap, wide tap and tap_used written, and k_cum_refine reading them (capi_process.hip:439,
    FftChoice::wide_tap) - and the one-frame k_fft_psd<14> with its LDS tap at 513, where k_cum_refine reads the psd.
    max_listeners is 600 in both, so tap_stride > 512 and the tap_used entries past 512 exist.  513 slots also need a
    ninth gather row (k_listen.hip:709, grid.y = (n_slots + 63) / 64)."""
    c = Case(16384, 1, 256, slots, [("batch", 1024), ("batch", 1024)], seed=6100 + slots, max_listeners=600)
    c.run(capi).close()


# -- 2. crossing 512 slots inside a stream ---------------------------------------------------------------------------------

def test_crossing_512_slots_by_attach_then_holes(capi):
    """N = 16384: a 1024-frame batch at 512 slots (k_fft_r32, host/batch_plan.h fft_choice), sdr_attach of a 513th
    listener, a batch at 513 slots (k_fft_psd<14>: the pool is a high-water mark, capi_bank.hip:421), then three listeners
    detached - holes under the high-water mark, still 513 slots and still k_fft_psd<14> - and a third batch.  The
    cumulation and every decoder run across both switches."""
    steps = [("batch", 1024), ("attach", 0, 9000), ("batch", 1024),
             ("detach", 0, 5), ("detach", 0, 300), ("detach", 0, 511), ("batch", 1024)]
    c = Case(16384, 1, 256, 512, steps, seed=6200, max_listeners=600)
    c.run(capi).close()


def test_crossing_512_slots_inside_a_deferred_batch(capi):
    """N = 16384: a deferred 1024-frame batch whose FFT runs at 512 slots (k_fft_r32, wide tap), then sdr_attach_at
    binds listeners 513 and 514 at the cumulation boundaries 300 and 700 inside it, so its listen half gathers 514 slots
    (k_listen.hip:709, a ninth gather row; k_listen.hip:67, frames before tapped_from from the retained psd rows); the
    next deferred batch runs k_fft_psd<14> (host/batch_plan.h fft_choice: tap_n > kR32MaxTap) with every listener on the tap."""
    steps = [("defer", 1024, [(0, 4000, 300), (0, 9001, 700)]), ("defer", 1024, [])]
    c = Case(16384, 1, 256, 512, steps, seed=6300, max_listeners=600)
    c.run(capi).close()


# -- 3. kMaxLdsTap ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,listeners", [(8192, 4096), (8192, 4097), (16384, 4100)])
def test_lds_tap_capacity(capi, n, listeners):
    """The one-frame FFT kernel (k_fft_psd.hip:911, kDefaultFpw = 1) keeps its listeners' bins in LDS while
    n_tap <= kMaxLdsTap (k_fft_psd.hip:519 `lds_tap`, and the dynamic LDS size at :1003) and drains the tap from the
    stored psd row past it (:635, tap_frame).  4096 and 4097 listeners on one band of N = 8192 in two 512-frame batches,
    and 4100 at N = 16384 in two 1024-frame batches: the frame count would select k_fft_r32 there, and it is the slot
    count (fft_choice, tap_n > kR32MaxTap) that puts the tap on k_fft_psd<14> instead.  64 or 65 gather rows."""
    frames = 1024 if n == 16384 else 512
    c = Case(n, 1, 256, listeners, [("batch", frames), ("batch", frames)], seed=6400 + listeners)
    c.run(capi).close()


# -- 4. many bands --------------------------------------------------------------------------------------------------------------

def test_config5_whole_on_one_gpu(capi):
    """BASELINE config 5 whole on one GPU: 64 bands x N = 8192 x 16 listeners (1024 in all): grid.y = 64 in the FFT
    and noise kernels, 64 bands of frame records and ListenGeom frame bases.  Six eager 24-frame batches (capture needs
    the bank at a multiple of sdr_graph_batches(); the fifth straddles the cumulation boundary at frame 99), then one
    graph replay (capi_graph.hip:118 sdr_graph_capture, :237 sdr_graph_launch) of six more (the boundary at 199 inside
    its third batch).  Every band against its own oracle receiver."""
    import torch

    per = 24
    c = Case(8192, 64, 16, 16, [("batch", per)] * 12, seed=6500, free_last=False)
    c.run_oracle()
    bank = c.new_bank(capi, torch.cuda.Stream())
    K = bank.graph_batches
    assert K * per * 2 == c.total
    for k in range(K):
        a, e = k * per, (k + 1) * per
        batch = torch.stack([iq[a:e] for iq in c.dev_iq]).contiguous()
        torch.cuda.synchronize()  # (the input is written on torch's stream, the bank reads it on its own)
        bank.process_device(batch.data_ptr(), per)
        res = bank.poll(wait=True)
        assert res["batch_index"] == k
        c.check_polled(res, a, e)
        c.check_device(bank, a, e, k)
    bank.graph_capture(per)
    batches = [torch.stack([iq[(K + k) * per:(K + k + 1) * per] for iq in c.dev_iq]).contiguous() for k in range(K)]
    torch.cuda.synchronize()
    bank.graph_launch([x.data_ptr() for x in batches])
    for k in range(K):
        res = bank.poll(wait=True)
        a = (K + k) * per
        assert res["batch_index"] == K + k
        c.check_polled(res, a, a + per)
    bank.sync()
    assert bank.total_frames == c.total
    c.check_device(bank, c.total - per, c.total, 2 * K - 1, cumulations=False)
    c.check_end(bank, min_edges=8)
    bank.close()


def test_fft_r32_claim_counters_beyond_8_bands(capi):
    """k_fft_r32 on 24 bands x N = 16384 x 64-frame batches (host/batch_plan.h fft_choice: 64 * 24 >= 1024 frames per
    launch, 16 slots): a claim counter pair per band (k_fft_r32.hip:289 `steal + 2 * blockIdx.y`), put back to zero by
    each band's last workgroup (:574), over two launches."""
    c = Case(16384, 24, 16, 16, [("batch", 64), ("batch", 64)], seed=6600, free_last=False)
    c.run(capi, min_edges=5).close()


# -- 5. the small plan behind many late attaches ------------------------------------------------------------------------------

@pytest.mark.parametrize("n,n_bands,rate,early,late", [(8192, 1, RATE, 32, 320), (4096, 2, 192_000, 16, 200)])
def test_small_plan_many_late_attaches(capi, n, n_bands, rate, early, late):
    """B * N <= 8192 (capi_process.hip:168: the gather on the peaks stream): one deferred 1000-frame batch in which
    sdr_attach_at binds `late` listeners per band at the nine cumulation boundaries inside it - dozens of k_put_slots
    launches on the listen stream (capi_process.hip:149, flush_late_attached) - then two eager batches with every
    listener carried.  Each batch is polled only after the next one is enqueued, so the listen stream may still be
    behind when the next gather is issued on the peaks stream; every such gather waits for the last put until the host
    has seen it done (capi_process.hip:358, slots_put_ev).  The oracle attaches each listener at its frame."""
    boundaries = list(range(100, 1000, 100))

    def steps(carriers):
        # the late listeners are the carriers after the first `early`, bound boundary by boundary, band by band
        late_steps = [(b, carriers[b][early + j], boundaries[j * len(boundaries) // late]) for b in range(n_bands) for j in range(late)]
        return [("defer", 1000, sorted(late_steps, key=lambda t: (t[2], t[0]))), ("batch", 1000), ("batch", 1000)]

    c = Case(n, n_bands, early + late, early, steps, seed=6700 + n, rate=rate, total_frames=3000)
    c.run(capi, lag=True).close()
