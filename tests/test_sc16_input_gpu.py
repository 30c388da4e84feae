"""sc16 input (complex int16, include/sdrainer_hip.h *_sc16) on the GPU.  A bank fed int16 frames must produce exactly
what a bank fed float32(x) / 32767 produces: every psd row, every frame record and every delivery (peaks, edges, runes,
with listeners attached), over the kernels the format reaches - k_fft_psd_sc16<9..14> and k_fft_r32_sc16 - and over
graph replay, staged host input and a group.  Band 0's psd rows also equal the CPU oracle.

The input is quantised synth.make_band output, scaled so that the noise spans hundreds of LSBs, with full-scale values
(+-32767, -32768) and values where a plain multiply by 1/32767 rounds differently planted in every frame.  As in
tests/test_fft_r32_stealing.py, frame f of a batch is frame f % P of a pool of P frames (a fresh pool per batch), so the
oracle computes the pool only."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import oracle as orc  # noqa: E402
from parity_tools import capi, sc16_to_float32 as to_f32  # noqa: E402, F401 (capi: the fixture)
from sdrainer_amd import synth  # noqa: E402

POOL = 13
SCALE = 3.0e5  # noise sigma 1e-3 -> 300 LSB; a tone (0.1) -> 30 000
RATE = {512: 12000, 1024: 48000, 2048: 96000, 4096: 192000, 8192: 1_000_000, 16384: 2_000_000}


def multiply_wrong():
    """int16 values where x * float32(1/32767) is not the correctly rounded x / 32767."""
    v = np.arange(-32768, 32768).astype(np.float32)
    return np.arange(-32768, 32768)[(v * np.float32(1.0 / 32767.0)) != (v / np.float32(32767.0))].astype(np.int16)


SPECIAL = np.concatenate([np.array([32767, -32768, -32767, 0, 1, -1], np.int16), multiply_wrong()[::97]])


def pool(n, tones, seed):
    """P quantised frames [P, 2N] int16, the tones' bins, and the oracle's psd of each frame (uint32 [P, N])."""
    iq, bins, _ = synth.make_band(POOL, RATE[n], n, tones, seed=seed)
    q = np.clip(np.rint(iq.astype(np.float64) * SCALE), -32768, 32767).astype(np.int16)
    for p in range(POOL):
        pos = (p * 37 + np.arange(len(SPECIAL)) * 101) % (2 * n)
        q[p, pos] = SPECIAL
    psd = np.stack([orc.iq_to_spectrum_and_psd(to_f32(q[p]))[1] for p in range(POOL)]).view(np.uint32)
    return q, bins, psd


def batch(q, frames):
    return q[np.arange(frames) % POOL]


class Pair:
    """Bank A takes float32 through the float32 path, bank B the int16 through the sc16 path."""

    def __init__(self, capi, n, bands, frames, tones, listeners=None, **kw):
        self.n, self.bands = n, bands
        self.a = capi.Bank(RATE[n], n, n_bands=bands, max_batch_frames=frames, max_listeners=max(listeners or tones, 1), **kw)
        self.b = capi.Bank(RATE[n], n, n_bands=bands, max_batch_frames=frames, max_listeners=max(listeners or tones, 1), **kw)
        for bk in (self.a, self.b):
            bk.enable_results(True)

    def attach(self, bins_per_band, extra=0):
        for band, bins in enumerate(bins_per_band):
            for k in range(len(bins) + extra):
                bin_ = int(bins[k % len(bins)]) if k < len(bins) else (k * 7919) % self.n
                assert self.a.attach(band, bin_) == self.b.attach(band, bin_)

    def run(self, q):
        """q: int16 [bands, frames, 2N]."""
        frames = q.shape[1]
        ta = torch.from_numpy(to_f32(q)).cuda()
        tb = torch.from_numpy(np.ascontiguousarray(q)).cuda()
        torch.cuda.synchronize()
        self.a.process_device(ta.data_ptr(), frames)
        self.b.process_device_sc16(tb.data_ptr(), frames)
        self.a.sync()
        self.b.sync()
        self.check(frames)

    def check(self, frames, rows=True):
        for band in range(self.bands):
            if rows:
                for f in range(frames):
                    sa, pa = self.a.read_spectrum(band, f)
                    sb, pb = self.b.read_spectrum(band, f)
                    assert pa.tobytes() == pb.tobytes(), f"band {band} frame {f}: psd row differs"
                    assert sa.tobytes() == sb.tobytes(), f"band {band} frame {f}: spectrum row differs"
            assert self.a.read_frame_records(band).tobytes() == self.b.read_frame_records(band).tobytes(), f"band {band}: frame records"
        same_deliveries(self.a, self.b)

    def close(self):
        self.a.close()
        self.b.close()


def same_deliveries(a, b):
    n = 0
    while True:
        da, db = a.poll(wait=False), b.poll(wait=False)
        assert (da is None) == (db is None)
        if da is None:
            break
        for k in ("batch_index", "first_frame", "n_frames", "runes_dropped", "edges_dropped"):
            assert da[k] == db[k], k
        for k in ("chunks", "peaks", "listeners", "edges", "runes", "rune_frames"):
            assert da[k].tobytes() == db[k].tobytes(), k
        n += 1
    return n


def check_oracle(bank, band, frames, want):
    for f in range(frames):
        _, psd = bank.read_spectrum(band, f)
        assert np.array_equal(psd.view(np.uint32), want[f % POOL]), f"band {band} frame {f}: psd differs from the oracle"


def test_input_has_the_hard_values():
    q, _, _ = pool(512, 4, 1)
    vals = set(np.unique(q).tolist())
    assert {32767, -32768, -32767} <= vals
    assert len(vals & set(multiply_wrong().tolist())) >= 10
    assert np.std(q.astype(np.float64)) > 300  # the samples span hundreds of LSBs at least


@pytest.mark.parametrize("n", [512, 1024, 2048, 4096, 8192, 16384])
def test_sizes_two_bands_consecutive(capi, n):
    """k_fft_psd_sc16<LOGN> (short batches: at N = 16384 the 16-point kernel): two bands, odd batch sizes, two batches."""
    tones = 6
    p = Pair(capi, n, 2, 45, tones)
    pools = [pool(n, tones, 100 + n + b) for b in range(2)]
    p.attach([pools[0][1], pools[1][1]])
    for i, frames in enumerate([45, 19]):
        if i:
            pools = [pool(n, tones, 200 + n + b) for b in range(2)]
        p.run(np.stack([batch(pools[b][0], frames) for b in range(2)]))
        check_oracle(p.b, 0, frames, pools[0][2])
    p.close()


def test_r32_long_batches(capi):
    """N = 16384, >= 1024 frames, <= 512 listeners: k_fft_r32_sc16; odd sizes, consecutive batches, then two bands."""
    n, tones = 16384, 8
    p = Pair(capi, n, 1, 1031, tones)
    q, bins, want = pool(n, tones, 300)
    p.attach([bins])
    p.run(batch(q, 1031)[None])
    check_oracle(p.b, 0, 1031, want)
    q, _, want = pool(n, tones, 301)
    p.run(batch(q, 1024)[None])
    check_oracle(p.b, 0, 1024, want)
    p.close()
    p = Pair(capi, n, 2, 515, tones)
    pools = [pool(n, tones, 310 + b) for b in range(2)]
    p.attach([pools[0][1], pools[1][1]])
    p.run(np.stack([batch(pools[b][0], 515) for b in range(2)]))
    check_oracle(p.b, 1, 515, pools[1][2])
    p.close()


def test_many_listeners(capi):
    """More than 512 listeners at N = 16384 and 1031 frames: k_fft_psd_sc16<14>; more than the LDS tap holds at N = 1024:
    the drain tap."""
    p = Pair(capi, 16384, 1, 1031, 8, listeners=600)
    q, bins, want = pool(16384, 8, 400)
    p.attach([bins], extra=600 - 8)
    p.run(batch(q, 1031)[None])
    check_oracle(p.b, 0, 1031, want)
    p.close()
    p = Pair(capi, 1024, 1, 33, 6, listeners=4100)
    q, bins, want = pool(1024, 6, 401)
    p.attach([bins], extra=4100 - 6)
    p.run(batch(q, 33)[None])
    check_oracle(p.b, 0, 33, want)
    p.close()


def test_graph_replay(capi):
    """sdr_graph_capture_sc16 / _launch_sc16 against the float32 graph, two replays; the other format's launch is
    SDR_ERR_STATE."""
    n, tones, frames = 4096, 6, 37
    p = Pair(capi, n, 1, frames, tones)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    p.a.set_stream(streams[0].cuda_stream)
    p.b.set_stream(streams[1].cuda_stream)
    q0, bins, _ = pool(n, tones, 500)
    p.attach([bins])
    K = p.a.graph_batches
    p.a.graph_capture(frames)
    p.b.graph_capture_sc16(frames)
    L = p.b._L
    for rep in range(2):
        pools = [pool(n, tones, 510 + rep * K + k) for k in range(K)]
        qs = [batch(pl[0], frames) for pl in pools]
        ta = [torch.from_numpy(to_f32(x)).cuda() for x in qs]
        tb = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in qs]
        torch.cuda.synchronize()
        arr_a = (C.c_void_p * K)(*[t.data_ptr() for t in ta])
        arr_b = (C.c_void_p * K)(*[t.data_ptr() for t in tb])
        assert L.sdr_graph_launch(p.b._h, arr_a) == 7  # SDR_ERR_STATE: captured for sc16
        assert L.sdr_graph_launch_sc16(p.a._h, arr_b) == 7  # SDR_ERR_STATE: captured for float32
        p.a.graph_launch([t.data_ptr() for t in ta])
        p.b.graph_launch_sc16([t.data_ptr() for t in tb])
        p.a.sync()
        p.b.sync()
        p.check(frames)  # (the read calls see the replay's last batch)
        check_oracle(p.b, 0, frames, pools[-1][2])
    arr_b = (C.c_void_p * K)(*([tb[0].data_ptr() + 2] + [t.data_ptr() for t in tb[1:]]))
    assert L.sdr_graph_launch_sc16(p.b._h, arr_b) == 1  # misaligned: SDR_ERR_BAD_ARG
    p.a.graph_release()
    p.b.graph_release()
    p.close()


def test_staged_push(capi):
    """sdr_push_iq_sc16 + sdr_process_staged equals sdr_push_iq of the converted values; rate, size, queue and mixing
    statuses."""
    from sdrainer_amd import capi as c
    n, tones, frames = 2048, 6, 40
    p = Pair(capi, n, 2, frames, tones)
    pools = [pool(n, tones, 600 + b) for b in range(2)]
    p.attach([pools[0][1], pools[1][1]])
    for rep in range(2):
        for b in range(2):
            x = batch(pools[b][0], frames)
            # in two pushes of 25 and 15 frames (the second batch leaves 10 staged frames over)
            for lo, hi in ((0, 25), (25, frames)):
                assert p.a.push_iq(b, RATE[n], to_f32(x[lo:hi])) == c.OK
                assert p.b.push_iq_sc16(b, RATE[n], x[lo:hi]) == c.OK
        assert p.a.process_staged_limit(frames - 10 * rep) == p.b.process_staged_limit(frames - 10 * rep) == frames - 10 * rep
        p.check(frames - 10 * rep)
    # the 10 frames left over, then the statuses
    assert p.a.process_staged() == p.b.process_staged() == 10
    p.check(10)
    x = pools[0][0]
    assert p.b.push_iq_sc16(0, RATE[n] + 1, x[:1]) == c.ERR_BAD_RATE
    assert p.b.push_iq_sc16(0, RATE[n], x[:1].ravel()[:-2]) == c.ERR_BAD_SIZE
    assert p.b.push_iq_sc16(0, RATE[n], np.zeros(0, np.int16)) == c.ERR_BAD_SIZE
    assert p.b.push_iq_sc16(0, RATE[n], batch(x, frames + 1)) == c.ERR_WOULD_DROP
    assert p.b._L.sdr_push_iq_sc16(p.b._h, 0, RATE[n], None, 2 * n) == c.ERR_BAD_ARG
    assert p.b._L.sdr_push_iq_sc16(p.b._h, 2, RATE[n], x[:1].ctypes.data_as(C.POINTER(C.c_int16)), 2 * n) == c.ERR_BAD_ARG
    assert p.b.push_iq_sc16(0, RATE[n], x[:2]) == c.OK
    assert p.b.push_iq(0, RATE[n], to_f32(x[:1])) == c.ERR_STATE
    snd = b"\0" * 17 + x[:1].astype(">i2").tobytes()
    assert p.b.push_kiwi_snd(0, RATE[n], snd) == c.ERR_STATE
    assert p.b.push_iq(1, RATE[n], to_f32(x[:1])) == c.OK
    assert p.b.push_iq_sc16(1, RATE[n], x[:1]) == c.ERR_STATE
    assert p.b.push_kiwi_snd(0 + 1, RATE[n], snd) == c.ERR_STATE
    assert p.b.staged_frames(0) == 2 and p.b.staged_frames(1) == 1
    p.close()


def test_group_equals_one_bank(capi):
    """A two-member group on device 0, sc16 by device pointers and by staged pushes, equals one bank of the same bands."""
    from sdrainer_amd import capi as c
    n, tones, frames, bands = 4096, 5, 31, 4
    bank = c.Bank(RATE[n], n, n_bands=bands, max_batch_frames=frames, max_listeners=tones)
    group = c.Group((0, 0), RATE[n], n, bands, max_batch_frames=frames, max_listeners=tones)
    bank.enable_results(True)
    group.enable_results(True)
    pools = [pool(n, tones, 700 + b) for b in range(bands)]
    for b in range(bands):
        m, lb = group.member(b)
        for bin_ in pools[b][1]:
            assert bank.attach(b, int(bin_)) == m.attach(lb, int(bin_))
    q = np.stack([batch(pools[b][0], frames) for b in range(bands)])
    t = torch.from_numpy(q).cuda()
    ts = [torch.from_numpy(np.ascontiguousarray(q[m::2])).cuda() for m in range(2)]
    torch.cuda.synchronize()
    bank.process_device_sc16(t.data_ptr(), frames)
    group.process_device_sc16([x.data_ptr() for x in ts], frames)
    for b in range(bands):
        assert bank.push_iq_sc16(b, RATE[n], q[b]) == c.OK
        assert group.push_iq_sc16(b, RATE[n], q[b]) == c.OK
    assert bank.process_staged() == group.process_staged() == frames
    bank.sync()
    group.sync()
    for b in range(bands):
        m, lb = group.member(b)
        for f in (0, frames - 1):
            assert bank.read_spectrum(b, f)[1].tobytes() == m.read_spectrum(lb, f)[1].tobytes()
    for _ in range(2):
        da, dg = bank.poll(wait=True), group.poll(wait=True)
        for k in ("batch_index", "first_frame", "n_frames", "runes_dropped", "edges_dropped"):
            assert da[k] == dg[k], k
        for k in ("chunks", "peaks", "listeners", "edges", "runes", "rune_frames"):
            assert da[k].tobytes() == dg[k].tobytes(), k
    L = group._L
    arr = (C.c_void_p * 2)(ts[0].data_ptr(), None)
    assert L.sdr_group_process_device_sc16(group._h, arr, frames) == c.ERR_BAD_ARG
    arr = (C.c_void_p * 2)(ts[0].data_ptr(), ts[1].data_ptr() + 4)
    assert L.sdr_group_process_device_sc16(group._h, arr, frames) == c.ERR_BAD_ARG
    assert L.sdr_group_process_device_sc16(group._h, None, frames) == c.ERR_BAD_ARG
    assert L.sdr_group_push_iq_sc16(group._h, bands, RATE[n], q[0].ctypes.data_as(C.POINTER(C.c_int16)), 2 * n) == c.ERR_BAD_ARG
    group.close()
    bank.close()


def test_bad_arguments(capi):
    from sdrainer_amd import capi as c
    bank = c.Bank(RATE[1024], 1024, max_batch_frames=8)
    L = bank._L
    t = torch.zeros(9 * 2 * 1024 + 8, dtype=torch.int16, device="cuda")
    assert L.sdr_process_device_sc16(None, C.c_void_p(t.data_ptr()), 1) == c.ERR_BAD_ARG
    assert L.sdr_process_device_sc16(bank._h, None, 1) == c.ERR_BAD_ARG
    assert L.sdr_process_device_sc16(bank._h, C.c_void_p(t.data_ptr() + 4), 1) == c.ERR_BAD_ARG
    assert L.sdr_process_device_sc16(bank._h, C.c_void_p(t.data_ptr()), 9) == c.ERR_BAD_ARG  # > max_batch_frames
    assert L.sdr_process_device_sc16(bank._h, C.c_void_p(t.data_ptr()), 0) == c.OK
    assert L.sdr_graph_launch_sc16(bank._h, None) == c.ERR_BAD_ARG
    assert L.sdr_graph_capture_sc16(bank._h, 9) == c.ERR_BAD_ARG
    arr = (C.c_void_p * bank.graph_batches)(*([t.data_ptr()] * bank.graph_batches))
    assert L.sdr_graph_launch_sc16(bank._h, arr) == c.ERR_STATE  # nothing captured
    bank.close()
