"""What the 8-bit input tests share (tests/test_iq8_inputs.py, tests/test_iq8_gpu.py): the two formats, the values a byte
stands for, the quantised input with every byte value planted, and the pair of banks the GPU tests compare.  A plain
helper module, not a test file: pytest does not rewrite its asserts, so each carries its own message.

Input: synth.make_band(..., noise_sigma=2e-2) times 120, rounded and clipped to [-128, 127]: the noise is 2.4 LSB, a tone
12 LSB.  (With the synth's default sigma the quantised noise windows are all zero, the noise floor is -Inf and nothing
is found: tests/test_iq8_inputs.py pins that this input is not that.)  cu8 is the same stream plus 128."""
import numpy as np

from oracle import oracle as orc
from sdrainer_amd import synth

CS8, CU8 = 0, 1  # SDR_IQ8_CS8, SDR_IQ8_CU8
FORMATS = [CS8, CU8]
FORMAT_IDS = ["cs8", "cu8"]
POOL = 13
SCALE = 120.0
SIGMA = 2e-2
RATE = {512: 12000, 1024: 48000, 2048: 96000, 4096: 192000, 8192: 1_000_000, 16384: 2_000_000, 32768: 2_000_000, 65536: 2_000_000}


def to_f32(x, fmt):
    """The float32 values the bytes stand for (include/sdrainer_hip.h): x / 128 for cs8, (x - 127.5) / 128 for cu8 - exact."""
    if fmt == CS8:
        return np.asarray(x, np.int8).astype(np.float32) / np.float32(128.0)
    return (np.asarray(x, np.uint8).astype(np.float32) - np.float32(127.5)) / np.float32(128.0)


def quantise(iq, fmt):
    """float32 samples -> bytes of format fmt (int8 / uint8 array of the same shape)."""
    q = np.clip(np.rint(np.asarray(iq, np.float64) * SCALE), -128, 127).astype(np.int16)
    return q.astype(np.int8) if fmt == CS8 else (q + 128).astype(np.uint8)


def plant_all_bytes(q, row):
    """Every one of the 256 byte values into the I and into the Q position of frame `q` [2N] (in place), at places that
    move with the frame's number `row`."""
    n = q.size // 2
    vals = np.arange(256).astype(np.uint8).view(q.dtype) if q.dtype == np.int8 else np.arange(256, dtype=np.uint8)
    at = (row * 37 + np.arange(256) * 2 + 1) % n  # 256 distinct samples (N >= 512)
    q[2 * at] = vals
    q[2 * ((at + 1) % n) + 1] = vals


def pool(n, tones, seed, fmt, frames=POOL, oracle_psd=True):
    """`frames` quantised frames [frames, 2N] of format fmt with all byte values planted, the tones' bins, and the oracle's
    psd of each frame (uint32 [frames, N]) or None."""
    iq, bins, _ = synth.make_band(frames, RATE[n], n, tones, seed=seed, noise_sigma=SIGMA)
    q = quantise(iq, fmt)
    for p in range(frames):
        plant_all_bytes(q[p], p)
    psd = None
    if oracle_psd:
        psd = np.stack([orc.iq_to_spectrum_and_psd(to_f32(q[p], fmt))[1] for p in range(frames)]).view(np.uint32)
    return q, bins, psd


def batch(q, frames):
    """Frame f of a batch is frame f % P of the pool."""
    return q[np.arange(frames) % len(q)]


def stream(n, hop, frames, tones, seed, fmt):
    """A continuous quantised stream [samples, 2] of format fmt holding `frames` frames of N at hop `hop`, and the carriers'
    bins of the N-point spectrum (synth.make_band row by row of one hop each is a continuous stream)."""
    n_hops = frames - 1 + n // hop
    iq, bins, _ = synth.make_band(n_hops, RATE[n], hop, tones, seed=seed, noise_sigma=SIGMA, free_last_window=True)
    q = quantise(iq, fmt)
    for p in range(min(n_hops, POOL)):
        plant_all_bytes(q[p], p)
    return q.reshape(-1, 2), [int(b) * (n // hop) for b in bins]


def same_deliveries(a, b):
    """Every delivery of banks a and b, byte for byte; returns how many there were."""
    n = 0
    while True:
        da, db = a.poll(wait=False), b.poll(wait=False)
        assert (da is None) == (db is None), "one bank delivered a batch the other did not"
        if da is None:
            return n
        for k in ("batch_index", "first_frame", "n_frames", "runes_dropped", "edges_dropped"):
            assert da[k] == db[k], k
        for k in ("chunks", "peaks", "listeners", "edges", "runes", "rune_frames"):
            assert da[k].tobytes() == db[k].tobytes(), k
        n += 1


class Pair:
    """Bank A takes float32 of the converted values through the float32 calls, bank B the bytes through the 8-bit calls."""

    def __init__(self, capi, n, bands, frames, tones, fmt, listeners=None, **kw):
        self.n, self.bands, self.fmt = n, bands, fmt
        mk = lambda: capi.Bank(RATE[n], n, n_bands=bands, max_batch_frames=frames, max_listeners=max(listeners or tones, 1), **kw)
        self.a, self.b = mk(), mk()
        for bk in (self.a, self.b):
            bk.enable_results(True)

    def attach(self, bins_per_band, extra=0):
        for band, bins in enumerate(bins_per_band):
            for k in range(len(bins) + extra):
                bin_ = int(bins[k % len(bins)]) if k < len(bins) else (k * 7919) % self.n
                ia, ib = self.a.attach(band, bin_), self.b.attach(band, bin_)
                assert ia == ib, "listener ids differ"

    def run(self, q):
        """q: bytes [bands, frames, 2N], dense frames."""
        import torch
        frames = q.shape[1]
        ta = torch.from_numpy(to_f32(q, self.fmt)).cuda()
        tb = torch.from_numpy(np.ascontiguousarray(q)).cuda()
        torch.cuda.synchronize()
        self.a.process_device(ta.data_ptr(), frames)
        self.b.process_device_iq8(tb.data_ptr(), frames, self.fmt)
        self.sync()
        self.check(frames)

    def sync(self):
        self.a.sync()
        self.b.sync()

    def check(self, frames, rows=True):
        for band in range(self.bands):
            if rows:
                for f in range(frames):
                    sa, pa = self.a.read_spectrum(band, f)
                    sb, pb = self.b.read_spectrum(band, f)
                    assert pa.tobytes() == pb.tobytes(), f"band {band} frame {f}: psd row differs"
                    assert sa.tobytes() == sb.tobytes(), f"band {band} frame {f}: spectrum row differs"
            assert self.a.read_frame_records(band).tobytes() == self.b.read_frame_records(band).tobytes(), f"band {band}: frame records"
        return same_deliveries(self.a, self.b)

    def close(self):
        self.a.close()
        self.b.close()


def check_oracle(bank, band, frames, want):
    for f in range(frames):
        _, psd = bank.read_spectrum(band, f)
        assert np.array_equal(psd.view(np.uint32), want[f % len(want)]), f"band {band} frame {f}: psd differs from the oracle"
