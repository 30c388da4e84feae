"""What the GPU parity tests share besides the Case driver (tests/parity_case.py): the `capi` fixture, bit comparisons,
the checks of one delivered batch and of what it leaves on the device, input streams and their oracle side, the tables
more than one file parametrises over, the pooled frames of the k_fft_r32 tests and the bank-beside-group pair.  A plain
helper module, not a test file: pytest does not rewrite its asserts, so each carries its own message."""
import contextlib
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
from numpy.lib.stride_tricks import sliding_window_view

from oracle import oracle as orc
from sdrainer_amd import synth

REC_FIELDS = ["min_mean", "variance", "dev_in", "nf_in", "noise_dev", "noise_floor", "peak_thr", "listen_thr"]
RATES = {512: 48_000, 4096: 192_000, 8192: 2_000_000, 16384: 2_000_000, 32768: 2_000_000, 65536: 2_000_000}

# Overlapped geometries (N, hop, frames per call and a shorter call behind it for everything that is carried, bands,
# carriers, listeners): chosen so that every FFT input path runs strided - k_fft_psd<LOGN> one frame per workgroup and its
# sc16 twin, k_fft_psd<14>, k_fft_r32 (1024 frames of N = 16384 and more) with the plain and, at 256 listeners, the wide
# tap, and k_fft2p_a
GEOMETRY = [
    (512, 128, (300, 130), 1, 6, 12),
    (4096, 1024, (700, 130), 1, 16, 24),
    (8192, 4096, (2048, 130), 8, 16, 16),
    (16384, 2048, (256, 130), 1, 16, 24),
    (16384, 4096, (1024, 130), 1, 16, 24),
    (16384, 4096, (2048, 130), 1, 256, 256),
    (32768, 8192, (256, 130), 1, 16, 24),
    (65536, 8192, (160, 130), 1, 16, 24),
]


@pytest.fixture(scope="module")
def capi():
    """The ctypes binding with the library built and loaded (imported by name into every module that uses it)."""
    from sdrainer_amd.csrc import build
    build.build()
    from sdrainer_amd import capi as c
    c.load()
    return c


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """(kernel name, FftKernel id, frames per workgroup) the batch plan picks, with the switches of the environment: the host
    helper tests/host/iq8_plan.cpp, asked for (n, frames, listener slots, windowed, format name, hop or 0)."""
    import subprocess

    exe = str(tmp_path_factory.mktemp("fft_plan") / "iq8_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(os.path.dirname(os.path.abspath(__file__)), "host", "iq8_plan.cpp")])

    def ask(n, frames, slots, windowed, fmt, hop):
        w = subprocess.check_output([exe, str(n), str(frames), "1", str(slots), str(int(windowed)), fmt, str(hop)], text=True).split()
        got = dict(zip(w[0::2], w[1::2]))
        return got["kernel"], int(got["id"]), int(got["frames_per_wg"])
    return ask


@contextlib.contextmanager
def environment(**kw):
    """Switches the library reads when a bank is created (host/batch_plan.h read_switches) or while it reads back."""
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# -- comparisons -----------------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def nan_equal_bits(a, b):
    """Bit for bit, except that two NaNs are equal whatever their sign and payload (which are not part of the contract)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return np.array_equal(np.where(both_nan, 0, a.view(u)), np.where(both_nan, 0, b.view(u)))


def assert_records_equal(got, want, what="", same=bits_equal):
    for f in REC_FIELDS:
        assert same(got[f], want[f]), f"{what} frame record field {f} differs"


def sc16_to_float32(q):
    """The float32 values an sc16 sample stands for (include/sdrainer_hip.h: float32(x) / 32767, one rounding)."""
    return np.asarray(q, np.int16).astype(np.float32) / np.float32(32767.0)


# -- input and its oracle side ---------------------------------------------------------------------------------------------
def make_stream(n, hop, frames, rate, tones, seed, sc16=False):
    """(float32 [samples, 2], int16 [samples, 2] or None, the carriers' bins of the N-point spectrum) of a stream that
    holds `frames` frames.  synth.make_band builds one frame per row, so make_band(n_hops, rate, hop, ...) flattened is a
    continuous stream: every tone makes whole cycles per hop, is keyed per hop, and bin i of the short transform is bin
    i * N / hop of the long one."""
    n_hops = frames - 1 + n // hop
    iq, bins, _ = synth.make_band(n_hops, rate, hop, tones, seed=seed, free_last_window=True)
    s = iq.reshape(-1, 2)
    q = None
    if sc16:
        q = np.rint(s.astype(np.float64) * (30000.0 / float(np.abs(s).max()))).astype(np.int16)
        s = sc16_to_float32(q)
    return s, q, [int(b) * (n // hop) for b in bins]


def frames_of(s, n, hop, a=0, e=None):
    """Frames [a, e) of stream s [samples, 2], materialised: float32 [frames, 2N]."""
    w = sliding_window_view(s, n, axis=0)[::hop][a:e]  # [frames, 2, N]
    return np.ascontiguousarray(w.transpose(0, 2, 1)).reshape(-1, 2 * n)


def windowed(frames, w, n):
    """Frames [F, 2N] float32 with sample i of each multiplied by w[i]: numpy's float32 product, one rounding per
    component - the definition of what the bank computes with that window."""
    w = np.asarray(w, np.float32)
    return (frames.reshape(-1, n, 2) * w[None, :, None]).astype(np.float32).reshape(-1, 2 * n)


def random_window(n, seed):
    """float32 in [0.25, 1): random and asymmetric, and large enough for the carriers to stand out as they did."""
    return (np.float32(0.25) + np.float32(0.75) * np.random.default_rng(seed).random(n, dtype=np.float32)).astype(np.float32)


def listener_bins(n, carriers, count):
    """The carriers, then both neighbours of each, then bins 0 and N - 1, up to `count` listeners."""
    out = list(carriers)
    for c in carriers:
        out += [c - 1, c + 1]
    out += [0, n - 1]
    return out[:count]


def decode(deb_col, rate, hop, stops=()):
    """oracle.Decoder(rate, hop) over one listener's debounced bits: text, state, and the tick that wrote each rune.  What
    means time follows the hop: the bank's decoders are cw.NewDecoder(sampleRate, hop), the oracle receiver's are built
    from the block size.  stops: ticks in front of which Decoder.stop() is called (sdr_listener_stop between two batches);
    what it writes is stamped with the tick before, the last one the listener took."""
    d = orc.Decoder(rate, hop)
    d.reset()
    L, col = orc.lib(), np.ascontiguousarray(deb_col, np.uint8)
    at, have = [], 0
    for f in range(len(col)):
        if f in stops:
            d.stop()
            now = L.orc_decoder_out_len(d._h)
            at += [f - 1] * (now - have)
            have = now
        L.orc_decoder_tick(d._h, int(col[f]))
        now = L.orc_decoder_out_len(d._h)
        at += [f] * (now - have)
        have = now
    return d.text(), d.state(), np.array(at, np.int64)


def run_oracle(rate, n, edge, bins_per_band, iq_per_band, centers, hop=None):
    """One oracle receiver per band over the whole input (frames [F, 2N]; with a hop, a stream [samples, 2] whose frames
    are materialised), bands in parallel.  Returns the receivers, their outputs and, with a hop, the hop-timed decoders
    of every listener (else None)."""
    refs = []
    for bins, cf in zip(bins_per_band, centers):
        r = orc.Receiver(rate, n, edge, 15.0, 1, center_frequency=cf)
        for b in bins:
            r.attach(int(b))
        refs.append(r)
    feed = iq_per_band if hop is None else [frames_of(s, n, hop) for s in iq_per_band]
    with ThreadPoolExecutor(max(1, min(len(refs), 16))) as ex:
        outs = list(ex.map(lambda ri: ri[0].process(ri[1]), zip(refs, feed)))
    decs = None if hop is None else [[decode(out["deb"][:, lid], rate, hop) for lid in range(len(bins))]
                                     for out, bins in zip(outs, bins_per_band)]
    return refs, outs, decs


# -- one batch against the oracle ------------------------------------------------------------------------------------------
def transitions(deb_col, a, e):
    deb = deb_col.astype(np.int8)
    trans = np.flatnonzero(np.diff(np.concatenate([[0], deb])) != 0)
    trans = trans[(trans >= a) & (trans < e)]
    return trans, deb[trans]


def peaks_of(res, ch):
    return [tuple(int(p[k]) if k != "signal_value" else float(p[k]) for k in
                  ("from", "to", "from_frequency", "to_frequency", "signal_frequency", "signal_value", "signal_bin"))
            for p in res["peaks"][ch["first_peak"]:ch["first_peak"] + ch["n_peaks"]]]


def frames32(frames, first_frame=0):
    """Stream frames as a bank that started at first_frame hands them out in its 32-bit fields (sdr_edge.frame,
    rune_frames): shifted, then reduced modulo 2^32.  int64, so that it compares with either."""
    return (np.asarray(frames, np.int64) + int(first_frame)) & 0xFFFFFFFF


def check_batch_polled(res, outs, a, e, tones, text, n_bands, live=None, gone=(), rune_at=None, max_peaks=None, edges_dropped=0,
                       first_frame=0, slot=None):
    """One polled batch (sdr_poll: what bench.py's consumer thread receives) against the oracle's whole-run output.
    live[band]: the listener ids to check (default: 0 .. tones - 1); gone: (band, listener) pairs detached before the
    batch, which must deliver nothing.  The runes go to text[band][listener], their frames to rune_at (if given).
    max_peaks: the bank's (None: it holds every run) - a cumulation delivers the oracle's first max_peaks peaks and says in
    peaks_found how many runs there were; every chunk's first_peak follows on the one before.  first_frame: the bank's
    (sdr_set_first_frame); a, e and the oracle count from 0, the batch's first_frame and chunk frames are expected shifted
    by it, edge frames shifted and modulo 2^32 (frames32), and rune_at collects the 32-bit rune frames as delivered.
    slot[band][listener]: the bank's id of the oracle's listener (default: the same; they differ once an attach has reused a
    detached listener's id).  Returns the edges and peaks delivered."""
    k = res["batch_index"]
    sl = (lambda band, lid: lid) if slot is None else (lambda band, lid: slot[band][lid])
    assert res["first_frame"] == first_frame + a and res["n_frames"] == e - a, \
        f"batch {k}: frames {res['first_frame']} + {res['n_frames']}, not [{a}, {e}) from {first_frame}"
    assert res["runes_dropped"] == 0 and res["edges_dropped"] == edges_dropped, f"batch {k}: runes or edges dropped"
    by = {(int(r["band"]), int(r["listener"])): r for r in res["listeners"]}
    for key in gone:
        r = by.get((key[0], sl(*key)))
        assert r is None or (r["n_edges"] == 0 and r["n_runes"] == 0), f"band {key[0]} listener {key[1]} batch {k}: delivers after its detach"
    n_edges = 0
    for band in range(n_bands):
        out = outs[band]
        for lid in (range(tones) if live is None else live[band]):
            trans, states = transitions(out["deb"][:, lid], a, e)
            r = by.get((band, sl(band, lid)))
            if r is None:
                assert len(trans) == 0, f"band {band} listener {lid} batch {k}: edges missing"
                continue
            ed = res["edges"][r["first_edge"]:r["first_edge"] + r["n_edges"]]
            assert np.array_equal(ed["frame"].astype(np.int64), frames32(trans, first_frame)) and np.array_equal(ed["state"], states), \
                f"band {band} listener {lid} batch {k} edges"
            n_edges += len(trans)
            runes = slice(r["first_rune"], r["first_rune"] + r["n_runes"])
            text[band][lid] += "".join(chr(int(x)) for x in res["runes"][runes])
            if rune_at is not None:
                rune_at[band][lid] += [int(x) for x in res["rune_frames"][runes]]
    n_peaks = 0
    seen = set()
    for ch in res["chunks"]:
        band = int(ch["band"])
        out = outs[band]
        assert ch["frame"].dtype == np.int64, "sdr_chunk_result.frame is 64-bit"
        gc = list(out["peak_frames"]).index(int(ch["frame"]) - first_frame)
        got, want = peaks_of(res, ch), out["peaks"][gc]
        stored = len(want) if max_peaks is None else min(len(want), max_peaks)
        assert ch["first_peak"] == n_peaks, f"band {band} batch {k} cumulation {gc}: first_peak {ch['first_peak']} after {n_peaks} peaks"
        assert ch["n_peaks"] == stored and ch["peaks_found"] == len(want), \
            f"band {band} batch {k} cumulation {gc}: {ch['n_peaks']} peaks of {ch['peaks_found']} found, not {stored} of {len(want)}"
        assert got == want[:stored], f"band {band} batch {k} peaks of cumulation {gc}"
        n_peaks += len(got)
        seen.add((band, gc))
    want = {(band, gc) for band in range(n_bands) for gc, f in enumerate(outs[band]["peak_frames"]) if a <= f < e}
    assert seen == want, f"batch {k}: cumulations (band, index) delivered {sorted(seen)}, completed {sorted(want)}"
    assert n_peaks == len(res["peaks"]), f"batch {k}: {len(res['peaks'])} peak records for {n_peaks} peaks"
    return n_edges, n_peaks


def check_device_batch(bank, outs, a, e, n_bands, live, k, cumulations=True, same=None, max_peaks=None, slot=None):
    """What the last batch [a, e) left on the device against the oracle: frame records, the keying bits of the listeners
    live[band], and (cumulations) every cumulation row it completed with its peaks (max_peaks: the bank's, by default read
    from it - sdr_read_peaks hands out the oracle's first max_peaks peaks and the number of runs found).  same: how two
    float arrays compare (default: bit for bit; streams that hold NaN pass one that lets NaN equal NaN).  slot: as in
    check_batch_polled."""
    same = same or bits_equal
    max_peaks = bank.cfg.max_peaks if max_peaks is None else max_peaks
    for b in range(n_bands):
        recs = bank.read_frame_records(b)
        for f in REC_FIELDS:
            assert same(recs[f], outs[b]["frames"][f][a:e].copy()), f"band {b} batch {k} field {f}"
        for lid in live[b]:
            assert np.array_equal(bank.read_keying_bits(b, lid if slot is None else slot[b][lid]), outs[b]["deb"][a:e, lid]), \
                f"band {b} listener {lid} batch {k}"
        if not cumulations:
            continue
        for c in range(bank.last_batch_chunks):
            pk, found, fr = bank.read_peaks(b, c)
            gc = list(outs[b]["peak_frames"]).index(a + fr)
            exact, want = outs[b]["cumulation"][gc], outs[b]["peaks"][gc]
            assert pk == want[:max_peaks] and found == len(want), \
                f"band {b} batch {k} cumulation {gc}: {len(pk)} peaks read of {found} found, the oracle has {len(want)}"
            assert bits_equal(bank.read_cumulation(b, c), exact), f"band {b} batch {k} cumulation {gc}"
            # the row as the pipeline keeps it (k_peaks.hip: exact where FindPeaks reads it, an upper bound elsewhere):
            # never below the exact cumulation in any bin, equal to it in every bin of every peak and beside its maximum
            with environment(SDR_READ_CUM_RAW=1):
                raw = bank.read_cumulation(b, c)
            assert np.all(raw >= exact), f"band {b} batch {k} cumulation {gc}: the kept row is below the exact one somewhere"
            # (beside the maximum also where that is outside the run - PeakCenterCorrection reads those two bins whatever the run
            # is, and a single-bin run has both outside; the refinement knows no max_peaks: exact at the truncated peaks too)
            for p in pk + want[max_peaks:]:
                lo, hi = max(0, p[6] - 1), min(len(exact) - 1, p[6] + 1)
                assert bits_equal(raw[p[0]:p[1] + 1], exact[p[0]:p[1] + 1]) and bits_equal(raw[lo:hi + 1], exact[lo:hi + 1]), \
                    f"band {b} batch {k} cumulation {gc}: the kept row differs from the exact one in peak {p[0]} - {p[1]}"


# -- pooled frames: the k_fft_r32 tests (tests/test_fft_r32_stealing.py, test_fft_reserve_gpu.py, queue_probe_case.py) -------
POOL_N = 16384
POOL_RATE = 2_000_000
POOL = 61


def pool_frames(seed):
    """P frames of noise and a tone at a random bin (float32 [P, 2N]) and the oracle's psd of each (uint32 [P, N])."""
    N = POOL_N
    rng = np.random.default_rng(seed)
    n = np.arange(N)
    iq = np.empty((POOL, 2 * N), np.float32)
    for p in range(POOL):
        k = rng.integers(N)
        iq[p, 0::2] = 0.2 * np.cos(2 * np.pi * k * n / N) + rng.normal(0, 1e-2, N)
        iq[p, 1::2] = 0.2 * np.sin(2 * np.pi * k * n / N) + rng.normal(0, 1e-2, N)
    psd = np.stack([orc.iq_to_spectrum_and_psd(iq[p])[1] for p in range(POOL)]).view(np.uint32)
    return iq, psd


def pool_batch(pool_dev, n_frames):
    """[n_frames, 2N] on the GPU: frame f = pool frame f % P."""
    import torch
    idx = torch.arange(n_frames, device=pool_dev.device) % POOL
    return pool_dev[idx].contiguous()


def check_pool_rows(bank, band, n_frames, want):
    psd = np.empty(POOL_N, np.float32)
    for f in range(n_frames):
        rc = bank._L.sdr_read_spectrum(bank._h, band, f, None, C.c_void_p(psd.ctypes.data))
        assert rc == 0, bank._L.sdr_last_error().decode()
        assert np.array_equal(psd.view(np.uint32), want[f % POOL]), f"band {band} frame {f}: psd row differs from the oracle"


def pool_bank(capi, n_bands, max_frames):
    return capi.Bank(POOL_RATE, POOL_N, n_bands=n_bands, max_batch_frames=max_frames, max_listeners=4, max_peaks=64)


# -- a bank beside a group of the same bands (tests/test_group_gpu.py, test_window_gpu.py) ----------------------------------
GROUP_BANDS = 5
GROUP_CENTER = [7_000_000 + 250_000 * b for b in range(GROUP_BANDS)]


def group_bands(frames, rate, n, tones, seed):
    out = [synth.make_band(frames, rate, n, tones, seed=seed + b) for b in range(GROUP_BANDS)]
    return np.stack([o[0] for o in out]), [o[1] for o in out]


def same_delivery(a, b):
    """Two deliveries (capi poll dicts), field by field, floats by their bits."""
    assert a is not None and b is not None, "a delivery is missing"
    i = a["batch_index"]
    for k in ("batch_index", "first_frame", "n_frames", "runes_dropped", "edges_dropped"):
        assert a[k] == b[k], f"batch {i} field {k}: {a[k]} != {b[k]}"
    for k in ("chunks", "peaks", "listeners", "edges", "runes", "rune_frames"):
        assert a[k].shape == b[k].shape, f"batch {i} field {k}: {a[k].shape[0]} records != {b[k].shape[0]}"
        assert a[k].tobytes() == b[k].tobytes(), f"batch {i} field {k} differs"


class Pair:
    """One bank of n_bands bands (GROUP_BANDS unless given) and a group of the same bands, fed the same input."""

    def __init__(self, capi, devices, rate, n, n_bands=GROUP_BANDS, **kw):
        import torch

        self.capi, self.devices, self.n = capi, devices, n
        self.bank = capi.Bank(rate, n, n_bands=n_bands, device_id=0, **kw)
        self.group = capi.Group(devices, rate, n, n_bands, **kw)
        self.M = len(devices)
        for b in range(n_bands):
            self.bank.set_center_frequency(b, GROUP_CENTER[b])
            m, lb = self.group.member(b)
            m.set_center_frequency(lb, GROUP_CENTER[b])
        self.dev = torch.cuda.current_device()

    def member_input(self, iq):
        """iq [bands, frames, 2N] -> one device tensor per member, [local band][frame][2N]."""
        import torch

        return [torch.from_numpy(np.ascontiguousarray(iq[m::self.M])).to(f"cuda:{d}") for m, d in enumerate(self.devices)]

    def process(self, iq):
        import torch

        nf = iq.shape[1]
        t = torch.from_numpy(np.ascontiguousarray(iq)).to("cuda:0")
        ts = self.member_input(iq)
        self.bank.process_device(t.data_ptr(), nf)
        self.group.process_device([x.data_ptr() for x in ts], nf)
        self.check_device()
        self.group.sync()
        self.bank.sync()
        self.check_device()

    def attach(self, band, bin_):
        lid = self.bank.attach(band, int(bin_))
        m, lb = self.group.member(band)
        assert m.attach(lb, int(bin_)) == lid, f"band {band}: the group's listener id differs from the bank's {lid}"
        return lid

    def polls(self, wait=True):
        a, b = self.bank.poll(wait=wait), self.group.poll(wait=wait)
        self.check_device()
        if a is None:
            assert b is None, "the group delivers where the bank does not"
            return None
        same_delivery(b, a)
        return b

    def check_device(self):
        import torch

        assert torch.cuda.current_device() == self.dev, "the caller's current device changed"

    def close(self):
        self.group.close()
        self.bank.close()


# -- the demonstration a window exists for (tests/test_window_host.py pins its oracle half, test_window_gpu.py runs the bank) ---
DEMO = dict(rate=192_000, n=4096, hop=1024, edge=560, bin=2600, weak_amplitude=3e-4, weak_text="cq de dl1abc dl1abc dl1abc k",
            weak_repeats=2, weak_wpm=20, strong_amplitude=0.1, strong_bin=2588.5, strong_text="test w1aw w1aw test", strong_wpm=27,
            strong_edge_ms=5.0, sigma=1e-3, seed=5)


def _carrier(bin_, n, a, e):
    """cos and sin of the carrier at spectrum bin `bin_` (a multiple of 0.5) over samples [a, e): FFT index bin_ + N / 2
    (the spectrum is fft-shifted), the phase reduced in integers."""
    k2 = int(round(2 * bin_)) + n  # twice the FFT index
    ph = np.pi * ((k2 * np.arange(a, e, dtype=np.int64)) % (2 * n)) / n
    return np.cos(ph), np.sin(ph)


def demo_stream(neighbour):
    """float32 [samples, 2]: the weak keyed station on bin 2600, the strong neighbour ("carrier": unkeyed; "soft": keyed
    with raised-cosine edges) and noise, I drawn before Q over the whole stream."""
    d = DEMO
    rate, n = d["rate"], d["n"]
    dit = int(round(1.2 / d["weak_wpm"] * rate))
    key = np.repeat(np.concatenate([np.zeros(30, np.uint8), np.tile(synth.keying_pattern(d["weak_text"], 1), d["weak_repeats"])]), dit)
    samples = (len(key) + n + 8191) // 8192 * 8192
    key = np.concatenate([key, np.zeros(samples - len(key), np.uint8)]).astype(np.float64)
    if neighbour == "carrier":
        strong = np.ones(samples)
    else:
        sdit = int(round(1.2 / d["strong_wpm"] * rate))
        pat = np.repeat(np.concatenate([synth.keying_pattern(d["strong_text"], 1), np.zeros(7, np.uint8)]), sdit)
        strong = np.tile(pat, samples // len(pat) + 1)[:samples].astype(np.float64)
        kern = np.hanning(int(round(d["strong_edge_ms"] * 1e-3 * rate)) + 2)[1:-1]
        strong = np.convolve(strong, kern / kern.sum(), mode="same")
    rng = np.random.default_rng(d["seed"])
    noise_i = d["sigma"] * rng.standard_normal(samples)
    noise_q = d["sigma"] * rng.standard_normal(samples)
    out = np.empty((samples, 2), np.float32)
    step = 1 << 21
    for a in range(0, samples, step):
        e = min(samples, a + step)
        wc, ws = _carrier(d["bin"], n, a, e)
        sc, ss = _carrier(d["strong_bin"], n, a, e)
        out[a:e, 0] = d["weak_amplitude"] * key[a:e] * wc + d["strong_amplitude"] * strong[a:e] * sc + noise_i[a:e]
        out[a:e, 1] = d["weak_amplitude"] * key[a:e] * ws + d["strong_amplitude"] * strong[a:e] * ss + noise_q[a:e]
    return out


def demo_oracle(s, w, piece=1200):
    """The oracle receiver (find_peaks on) over every frame of stream s with window w (None: rectangular), the frames
    materialised `piece` at a time, and the hop-timed decoder over the listener's debounced bits.  Returns deb bits, text,
    decoder state, and per completed cumulation its completing frame and peak list."""
    d = DEMO
    rate, n, hop = d["rate"], d["n"], d["hop"]
    r = orc.Receiver(rate, n, d["edge"])
    r.attach(d["bin"])
    frames = (s.shape[0] - n) // hop + 1
    deb, peak_frames, peaks = [], [], []
    for a in range(0, frames, piece):
        f = frames_of(s, n, hop, a, min(a + piece, frames))
        out = r.process(f if w is None else windowed(f, w, n))
        deb.append(out["deb"][:, 0])
        peak_frames += [a + int(x) for x in out["peak_frames"]]
        peaks += out["peaks"]
    deb = np.concatenate(deb)
    text, state, _ = decode(deb, rate, hop)
    return dict(deb=deb, text=text, state=state, peak_frames=peak_frames, peaks=peaks, frames=frames)


def merged_runs(peaks, lo=2588, hi=2600):
    """How many cumulations hold one peak run that contains both bins (the two stations are one peak), and the longest run."""
    merged = sum(any(p[0] <= lo and p[1] >= hi for p in pk) for pk in peaks)
    longest = max((p[1] - p[0] + 1 for pk in peaks for p in pk), default=0)
    return merged, longest


def check_demo_oracle(rect, hann):
    """The assertions on the oracle alone: they come first, so that a weak input fails as an input."""
    assert len(rect["peaks"]) == len(hann["peaks"]) >= 70, (len(rect["peaks"]), len(hann["peaks"]))
    assert "dl1abc" not in rect["text"], rect["text"]
    assert merged_runs(rect["peaks"])[0] * 2 >= len(rect["peaks"]), merged_runs(rect["peaks"])
    assert hann["text"].count("dl1abc") >= 4, hann["text"]
    assert merged_runs(hann["peaks"])[0] == 0, merged_runs(hann["peaks"])
