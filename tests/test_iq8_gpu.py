"""8-bit input (cs8 / cu8, include/sdrainer_hip.h *_iq8) on the GPU.  A bank fed bytes must produce exactly what a bank fed
the float32 values those bytes stand for produces: every psd and spectrum row, every frame record and every delivery
(peaks, edges, runes, with listeners attached), over the kernels the formats reach - k_fft_psd_iq8<9..14> plain and
windowed, k_fft_r32_iq8 and its strided form, k_fft2p_a's 8-bit instances, k_unpack_iq8 - and over streams with a hop,
graph replay, staged host input, a group, waterfall rows and listener reports.  Band 0's psd rows also equal the CPU
oracle's.  Every test runs for both formats (test_staged_kinds_side_by_side holds both, and the other staged kinds, in one bank).

The input is tests/iq8_tools.py's (tests/test_iq8_inputs.py shows that the oracle hears it).  As in
tests/test_sc16_input_gpu.py, frame f of a dense batch is frame f % P of a pool of P frames (a fresh pool per batch), so
the oracle computes the pool only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import iq8_tools as t8  # noqa: E402
from iq8_tools import RATE, Pair, batch, check_oracle, pool, to_f32  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from parity_tools import capi, frames_of, random_window, sc16_to_float32, windowed  # noqa: E402, F401 (capi: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
both = pytest.mark.parametrize("fmt", t8.FORMATS, ids=t8.FORMAT_IDS)


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """The FFT kernel family the batch plan picks for a geometry (tests/host/iq8_plan.cpp over host/batch_plan.h)."""
    exe = str(tmp_path_factory.mktemp("iq8_plan") / "iq8_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "host", "iq8_plan.cpp")])

    def ask(n, frames, bands, slots, windowed_=False):
        w = subprocess.check_output([exe, str(n), str(frames), str(bands), str(slots), str(int(windowed_))], text=True).split()
        return dict(zip(w[0::2], (int(x) for x in w[1::2])))
    return ask


@both
@pytest.mark.parametrize("n", [512, 1024, 2048, 4096, 8192, 16384])
def test_sizes_two_bands_consecutive(capi, planned, n, fmt):
    """k_fft_psd_iq8<LOGN> (short batches: at N = 16384 the 16-point kernel): two bands, odd batch sizes, two batches."""
    tones = 6
    assert planned(n, 45, 2, tones) == {"r32": 0, "wide_tap": 0, "two_phase": 0}
    p = Pair(capi, n, 2, 45, tones, fmt)
    pools = [pool(n, tones, 100 + n + b, fmt) for b in range(2)]
    p.attach([pools[0][1], pools[1][1]])
    for i, frames in enumerate([45, 19]):
        if i:
            pools = [pool(n, tones, 200 + n + b, fmt) for b in range(2)]
        p.run(np.stack([batch(pools[b][0], frames) for b in range(2)]))
        check_oracle(p.b, 0, frames, pools[0][2])
    p.close()


@both
def test_r32_long_batches(capi, planned, fmt):
    """N = 16384, >= 1024 frames, <= 512 listeners: k_fft_r32_iq8 (the plan says so); odd sizes, consecutive batches, then
    two bands."""
    n, tones = 16384, 8
    for frames, bands in ((1031, 1), (1024, 1), (515, 2)):
        assert planned(n, frames, bands, tones)["r32"] == 1
    p = Pair(capi, n, 1, 1031, tones, fmt)
    q, bins, want = pool(n, tones, 300, fmt)
    p.attach([bins])
    p.run(batch(q, 1031)[None])
    check_oracle(p.b, 0, 1031, want)
    q, _, want = pool(n, tones, 301, fmt)
    p.run(batch(q, 1024)[None])
    check_oracle(p.b, 0, 1024, want)
    p.close()
    p = Pair(capi, n, 2, 515, tones, fmt)
    pools = [pool(n, tones, 310 + b, fmt) for b in range(2)]
    p.attach([pools[0][1], pools[1][1]])
    p.run(np.stack([batch(pools[b][0], 515) for b in range(2)]))
    check_oracle(p.b, 0, 515, pools[0][2])
    check_oracle(p.b, 1, 515, pools[1][2])
    p.close()


@both
def test_many_listeners(capi, planned, fmt):
    """More than 512 listeners at N = 16384 and 1031 frames: k_fft_psd_iq8<14>; more than the LDS tap holds at N = 1024:
    the tap that re-reads the stored row."""
    assert planned(16384, 1031, 1, 600)["r32"] == 0
    p = Pair(capi, 16384, 1, 1031, 8, fmt, listeners=600)
    q, bins, want = pool(16384, 8, 400, fmt)
    p.attach([bins], extra=600 - 8)
    p.run(batch(q, 1031)[None])
    check_oracle(p.b, 0, 1031, want)
    p.close()
    p = Pair(capi, 1024, 1, 33, 6, fmt, listeners=4100)
    q, bins, want = pool(1024, 6, 401, fmt)
    p.attach([bins], extra=4100 - 6)
    p.run(batch(q, 33)[None])
    check_oracle(p.b, 0, 33, want)
    p.close()


@both
@pytest.mark.parametrize("n", [32768, 65536])
def test_wide_blocks(capi, planned, n, fmt):
    """N = 32768 and 65536: k_fft2p_a's 8-bit instances in front of phase B; 3 frames, two bands, 4 listeners."""
    tones, frames = 4, 3
    assert planned(n, frames, 2, tones)["two_phase"] == 1
    p = Pair(capi, n, 2, frames, tones, fmt)
    pools = [pool(n, tones, 450 + b, fmt, frames=frames) for b in range(2)]
    p.attach([pools[0][1], pools[1][1]])
    p.run(np.stack([pools[b][0] for b in range(2)]))
    check_oracle(p.b, 0, frames, pools[0][2])
    p.close()


def stream_pair(capi, n, hop, frames, tones, fmt, seed, window=None, listeners=None):
    """A pair of one-band banks with hop `hop`, the stream on the device in both forms, and the oracle's frames."""
    q, bins = t8.stream(n, hop, frames, tones, seed, fmt)
    p = Pair(capi, n, 1, frames, tones, fmt, listeners=listeners, hop=hop)
    if window is not None:
        p.a.set_window(window)
        p.b.set_window(window)
    p.attach([bins])
    s = to_f32(q, fmt)
    return p, torch.from_numpy(s).cuda(), torch.from_numpy(np.ascontiguousarray(q)).cuda(), s


def stream_calls(p, da, db, n, hop, cuts, s, fmt, window=None, every=1):
    """Frames [cuts[i], cuts[i + 1]) in one stream call each; after each, both banks compared and band 0 held to the oracle."""
    samples = da.shape[0]
    assert samples % 8 == 0
    torch.cuda.synchronize()
    for a, e in zip(cuts[:-1], cuts[1:]):
        left = samples - a * hop
        p.a.process_device_stream(da.data_ptr() + a * hop * 8, e - a, left)
        p.b.process_device_stream_iq8(db.data_ptr() + a * hop * 2, e - a, left, fmt)
        p.sync()
        p.check(e - a)
        picked = sorted(set(range(0, e - a, every)) | {e - a - 1})
        fr = np.stack([s[(a + f) * hop:(a + f) * hop + n].reshape(-1) for f in picked])
        if window is not None:
            fr = windowed(fr, window, n)
        for k, f in enumerate(picked):
            want = orc.iq_to_spectrum_and_psd(fr[k])[1].view(np.uint32)
            assert np.array_equal(p.b.read_spectrum(0, f)[1].view(np.uint32), want), f"frame {a + f}: psd differs from the oracle"


@both
def test_stream_two_calls(capi, fmt):
    """N = 2048, hop 512, 40 frames in two sdr_process_device_stream_iq8 calls cut at an odd frame; a band stride that is
    no multiple of 8 samples is refused."""
    n, hop, frames = 2048, 512, 40
    p, da, db, s = stream_pair(capi, n, hop, frames, 6, fmt, 800)
    stream_calls(p, da, db, n, hop, [0, 23, frames], s, fmt)
    L = p.b._L
    for stride in (da.shape[0] + 4, da.shape[0] + 1):
        assert L.sdr_process_device_stream_iq8(p.b._h, C.c_void_p(db.data_ptr()), 2, stride, fmt) == capi.ERR_BAD_ARG
    assert L.sdr_process_device_stream_iq8(p.b._h, C.c_void_p(db.data_ptr()), frames, 8, fmt) == capi.ERR_BAD_ARG  # shorter than the frames
    assert L.sdr_process_device_iq8(p.b._h, C.c_void_p(db.data_ptr()), 2, fmt) == capi.ERR_STATE  # the dense call on a bank with a hop
    p.close()


@both
def test_stream_r32_hop(capi, planned, fmt):
    """N = 16384, hop 4096, 1031 frames: k_fft_r32_hop_iq8."""
    n, hop, frames = 16384, 4096, 1031
    assert planned(n, frames, 1, 8)["r32"] == 1
    p, da, db, s = stream_pair(capi, n, hop, frames, 8, fmt, 810)
    stream_calls(p, da, db, n, hop, [0, frames], s, fmt, every=53)
    p.close()


@both
def test_stream_wide_block(capi, fmt):
    """N = 65536, hop 8192, 5 frames: k_fft2p_a's 8-bit instances with a frame stride."""
    n, hop, frames = 65536, 8192, 5
    p, da, db, s = stream_pair(capi, n, hop, frames, 4, fmt, 820)
    stream_calls(p, da, db, n, hop, [0, frames], s, fmt)
    p.close()


@both
def test_windowed(capi, fmt):
    """A random asymmetric window: N = 1024 dense (k_fft_psd_iq8's windowed twin) and N = 32768 with hop 4096
    (k_fft2p_a's windowed 8-bit instances), against bank A with the same table and the oracle on the windowed frames."""
    n, tones, frames = 1024, 6, 45
    w = random_window(n, 900)
    p = Pair(capi, n, 2, frames, tones, fmt)
    p.a.set_window(w)
    p.b.set_window(w)
    pools = [pool(n, tones, 901 + b, fmt, oracle_psd=False) for b in range(2)]
    p.attach([pools[0][1], pools[1][1]])
    p.run(np.stack([batch(pools[b][0], frames) for b in range(2)]))
    want = np.stack([orc.iq_to_spectrum_and_psd(x)[1] for x in windowed(to_f32(pools[0][0], fmt), w, n)]).view(np.uint32)
    check_oracle(p.b, 0, frames, want)
    p.close()
    n, hop, frames = 32768, 4096, 9
    w = random_window(n, 910)
    p, da, db, s = stream_pair(capi, n, hop, frames, 4, fmt, 911, window=w)
    stream_calls(p, da, db, n, hop, [0, 5, frames], s, fmt, window=w)
    p.close()


@both
@pytest.mark.parametrize("overlapped", [False, True], ids=["dense", "hop"])
def test_staged_push(capi, fmt, overlapped):
    """sdr_push_iq8 + sdr_process_staged equals sdr_push_iq of the converted values, pushed in uneven pieces, dense and with
    hop = N / 4 (only the new samples are uploaded)."""
    c = capi
    n, tones, frames = 2048, 6, 40
    hop = n // 4 if overlapped else n
    p = Pair(capi, n, 2, frames, tones, fmt, hop=hop if overlapped else 0)
    streams = [t8.stream(n, hop, 2 * frames, tones, 600 + b, fmt) for b in range(2)]
    p.attach([streams[0][1], streams[1][1]])
    hops = streams[0][0].shape[0] // hop
    at = 0
    for piece in (7, 30, 26, hops - 63):  # (in hops)
        for b in range(2):
            x = streams[b][0][at * hop:(at + piece) * hop]
            assert p.a.push_iq(b, RATE[n], to_f32(x, fmt)) == c.OK
            assert p.b.push_iq8(b, RATE[n], x, fmt) == c.OK
        at += piece
        fa, fb = p.a.staged_frames(0), p.b.staged_frames(0)
        assert fa == fb
        if fa >= 17:
            want = min(fa, frames) - 3  # (leaves staged frames over)
            assert p.a.process_staged_limit(want) == p.b.process_staged_limit(want) == want
            p.sync()
            p.check(want)
    left = p.a.staged_frames(0)
    assert left > 0 and p.a.process_staged() == p.b.process_staged() == left
    p.sync()
    p.check(left)
    # the last frame against the oracle
    s = to_f32(streams[0][0], fmt)
    want = orc.iq_to_spectrum_and_psd(frames_of(s, n, hop)[-1])[1].view(np.uint32)
    assert np.array_equal(p.b.read_spectrum(0, left - 1)[1].view(np.uint32), want)
    p.close()


@pytest.mark.parametrize("overlapped", [False, True], ids=["dense", "hop"])
def test_staged_kinds_side_by_side(capi, overlapped):
    """Every kind of staged frames in one batch, a band each: float32, KiwiSDR payloads (dense frames only: sdr_push_kiwi_snd
    is refused with a hop), sc16, cs8, cu8, at N = 512 and max_batch_frames = 8 - the smallest shapes at which a wrong row
    offset of one kind lands in another kind's bytes.  Bank B gets each band in its own kind, bank A sdr_push_iq of the
    converted values; uneven pieces, every batch cut by sdr_process_staged_limit so that frames stay staged, seven batches
    (each of the three staging sets is reused).  After each batch every psd row of every band is the same float32 bits."""
    c = capi
    n, frames = 512, 8
    hop = n // 4 if overlapped else n
    kinds = ["f32", "sc16", "cs8", "cu8"] if overlapped else ["f32", "kiwi", "sc16", "cs8", "cu8"]
    pieces = (8 if overlapped else 5, 4, 6, 3, 5, 2)  # (in hops; two frames stay staged behind every batch)
    samples = sum(pieces) * hop
    rng = np.random.default_rng(660 + overlapped)
    mk = lambda: c.Bank(RATE[n], n, n_bands=len(kinds), max_batch_frames=frames, hop=hop if overlapped else 0)
    a, b = mk(), mk()
    raw = {"f32": rng.standard_normal((samples, 2)).astype(np.float32),
           "kiwi": rng.integers(-32768, 32768, size=(samples, 2)).astype(np.int16),
           "sc16": rng.integers(-32768, 32768, size=(samples, 2)).astype(np.int16),
           "cs8": rng.integers(-128, 128, size=(samples, 2)).astype(np.int8),
           "cu8": rng.integers(0, 256, size=(samples, 2)).astype(np.uint8)}

    def push(band, kind, x):
        """x [samples, 2] of the band's kind into bank B as it is, into bank A as the float32 values it stands for."""
        if kind == "f32":
            rc, ref = b.push_iq(band, RATE[n], x), x
        elif kind == "kiwi":
            payload = bytes([0x01] + [7] * 16) + x.astype(">i2").tobytes()
            rc, ref = b.push_kiwi_snd(band, RATE[n], payload), orc.decode_iq_message(payload)
        elif kind == "sc16":
            rc, ref = b.push_iq_sc16(band, RATE[n], x), sc16_to_float32(x)
        else:
            fmt = t8.CS8 if kind == "cs8" else t8.CU8
            rc, ref = b.push_iq8(band, RATE[n], x, fmt), to_f32(x, fmt)
        assert rc == c.OK and a.push_iq(band, RATE[n], ref) == c.OK, f"{kind}: push refused"

    def same_rows(count):
        a.sync()
        b.sync()
        for band, kind in enumerate(kinds):
            for f in range(count):
                pa, pb = a.read_spectrum(band, f)[1], b.read_spectrum(band, f)[1]
                assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), f"band {band} ({kind}) frame {f} of the batch: psd differs"
            assert np.all(np.isfinite(pb)) and np.any(pb > 0)

    at = batches = 0
    for piece in pieces:
        for band, kind in enumerate(kinds):
            push(band, kind, raw[kind][at * hop:(at + piece) * hop])
        at += piece
        staged = [bk.staged_frames(band) for bk in (a, b) for band in range(len(kinds))]
        assert min(staged) == max(staged) >= 3
        want = staged[0] - 2
        assert a.process_staged_limit(want) == b.process_staged_limit(want) == want
        same_rows(want)
        batches += 1
    assert a.process_staged() == b.process_staged() == 2
    same_rows(2)
    assert batches + 1 >= 5 and a.staged_frames(0) == b.staged_frames(0) == 0
    a.close()
    b.close()


@both
def test_staged_statuses(capi, fmt):
    """Rate, size, queue-full and every mixing refusal of sdr_push_iq8, the other 8-bit format included."""
    c = capi
    n, frames = 2048, 8
    other = t8.CU8 if fmt == t8.CS8 else t8.CS8
    bank = c.Bank(RATE[n], n, n_bands=2, max_batch_frames=frames)
    x, _, _ = pool(n, 4, 650, fmt, oracle_psd=False)
    L = bank._L
    ptr = C.c_void_p(x.ctypes.data)
    assert bank.push_iq8(0, RATE[n] + 1, x[:1], fmt) == c.ERR_BAD_RATE
    assert bank.push_iq8(0, RATE[n], x[:1].ravel()[:-2], fmt) == c.ERR_BAD_SIZE
    assert bank.push_iq8(0, RATE[n], x[:0], fmt) == c.ERR_BAD_SIZE
    assert bank.push_iq8(0, RATE[n], batch(x, frames + 1), fmt) == c.ERR_WOULD_DROP
    assert L.sdr_push_iq8(bank._h, 0, RATE[n], None, 2 * n, fmt) == c.ERR_BAD_ARG
    assert L.sdr_push_iq8(bank._h, 2, RATE[n], ptr, 2 * n, fmt) == c.ERR_BAD_ARG
    assert L.sdr_push_iq8(bank._h, 0, RATE[n], ptr, 2 * n, 2) == c.ERR_BAD_ARG
    assert L.sdr_push_iq8(bank._h, 0, RATE[n], ptr, 2 * n, -1) == c.ERR_BAD_ARG
    assert bank.staged_frames(0) == 0
    snd = b"\0" * 17 + bytes(4 * n)
    f32, s16 = to_f32(x[:1], fmt), np.zeros(2 * n, np.int16)
    # band 0 holds this format: nothing else goes in
    assert bank.push_iq8(0, RATE[n], x[:2], fmt) == c.OK
    assert bank.push_iq8(0, RATE[n], x[:1].view(np.uint8), other) == c.ERR_STATE
    assert bank.push_iq(0, RATE[n], f32) == c.ERR_STATE
    assert bank.push_iq_sc16(0, RATE[n], s16) == c.ERR_STATE
    assert bank.push_kiwi_snd(0, RATE[n], snd) == c.ERR_STATE
    # band 1 holds float32, then (after a batch) sc16, then KiwiSDR frames: the 8-bit push is refused behind each
    assert bank.push_iq(1, RATE[n], f32) == c.OK
    assert bank.push_iq8(1, RATE[n], x[:1], fmt) == c.ERR_STATE
    assert bank.staged_frames(0) == 2 and bank.staged_frames(1) == 1
    assert bank.process_staged() == 1
    assert bank.push_iq_sc16(1, RATE[n], s16) == c.OK
    assert bank.push_iq8(1, RATE[n], x[:1], fmt) == c.ERR_STATE
    assert bank.process_staged() == 1
    assert bank.push_kiwi_snd(1, RATE[n], snd) == c.OK
    assert bank.push_iq8(1, RATE[n], x[:1], fmt) == c.ERR_STATE
    assert bank.push_iq8(0, RATE[n], x[:1], fmt) == c.OK
    assert bank.process_staged() == 1
    # band 0 is empty again: the other 8-bit format may follow, and then refuses this one
    assert bank.push_iq8(0, RATE[n], x[:1].view(np.uint8), other) == c.OK
    assert bank.push_iq8(0, RATE[n], x[:1], fmt) == c.ERR_STATE
    bank.sync()
    bank.close()


@both
def test_graph_replay(capi, fmt):
    """sdr_graph_capture_iq8 / _launch_iq8 against the float32 graph, two replays, N = 1024, 20 frames; a launch with
    another format is SDR_ERR_STATE."""
    n, tones, frames = 1024, 6, 20
    other = t8.CU8 if fmt == t8.CS8 else t8.CS8
    p = Pair(capi, n, 1, frames, tones, fmt)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    p.a.set_stream(streams[0].cuda_stream)
    p.b.set_stream(streams[1].cuda_stream)
    _, bins, _ = pool(n, tones, 500, fmt, oracle_psd=False)
    p.attach([bins])
    K = p.a.graph_batches
    p.a.graph_capture(frames)
    p.b.graph_capture_iq8(frames, fmt)
    L = p.b._L
    for rep in range(2):
        pools = [pool(n, tones, 510 + rep * K + k, fmt) for k in range(K)]
        qs = [batch(pl[0], frames) for pl in pools]
        ta = [torch.from_numpy(to_f32(x, fmt)).cuda() for x in qs]
        tb = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in qs]
        torch.cuda.synchronize()
        arr_a = (C.c_void_p * K)(*[t.data_ptr() for t in ta])
        arr_b = (C.c_void_p * K)(*[t.data_ptr() for t in tb])
        assert L.sdr_graph_launch(p.b._h, arr_a) == capi.ERR_STATE  # captured for this 8-bit format
        assert L.sdr_graph_launch_sc16(p.b._h, arr_b) == capi.ERR_STATE
        assert L.sdr_graph_launch_iq8(p.b._h, arr_b, other) == capi.ERR_STATE
        assert t8.FORMAT_IDS[fmt] in capi.load().sdr_last_error().decode()  # (the message names the right call)
        assert L.sdr_graph_launch_iq8(p.a._h, arr_b, fmt) == capi.ERR_STATE  # captured for float32
        assert L.sdr_graph_launch_iq8(p.b._h, arr_b, 2) == capi.ERR_BAD_ARG
        p.a.graph_launch([t.data_ptr() for t in ta])
        p.b.graph_launch_iq8([t.data_ptr() for t in tb], fmt)
        p.sync()
        assert p.check(frames) > 0  # (the read calls see the replay's last batch)
        check_oracle(p.b, 0, frames, pools[-1][2])
    arr_b = (C.c_void_p * K)(*([tb[0].data_ptr() + 2] + [t.data_ptr() for t in tb[1:]]))
    assert L.sdr_graph_launch_iq8(p.b._h, arr_b, fmt) == capi.ERR_BAD_ARG  # misaligned
    p.a.graph_release()
    p.b.graph_release()
    p.close()


@both
def test_group_equals_one_bank(capi, fmt):
    """A two-member group on device 0, by device pointers and by staged pushes, equals one bank of the same three bands."""
    c = capi
    n, tones, frames, bands = 4096, 5, 31, 3
    bank = c.Bank(RATE[n], n, n_bands=bands, max_batch_frames=frames, max_listeners=tones)
    group = c.Group((0, 0), RATE[n], n, bands, max_batch_frames=frames, max_listeners=tones)
    bank.enable_results(True)
    group.enable_results(True)
    pools = [pool(n, tones, 700 + b, fmt) for b in range(bands)]
    for b in range(bands):
        m, lb = group.member(b)
        for bin_ in pools[b][1]:
            assert bank.attach(b, int(bin_)) == m.attach(lb, int(bin_))
    q = np.stack([batch(pools[b][0], frames) for b in range(bands)])
    t = torch.from_numpy(q).cuda()
    ts = [torch.from_numpy(np.ascontiguousarray(q[m::2])).cuda() for m in range(2)]
    torch.cuda.synchronize()
    bank.process_device_iq8(t.data_ptr(), frames, fmt)
    group.process_device_iq8([x.data_ptr() for x in ts], frames, fmt)
    for b in range(bands):
        assert bank.push_iq8(b, RATE[n], q[b], fmt) == c.OK
        assert group.push_iq8(b, RATE[n], q[b], fmt) == c.OK
    assert bank.process_staged() == group.process_staged() == frames
    bank.sync()
    group.sync()
    for b in range(bands):
        m, lb = group.member(b)
        for f in (0, frames - 1):
            assert bank.read_spectrum(b, f)[1].tobytes() == m.read_spectrum(lb, f)[1].tobytes()
    check_oracle(bank, 0, frames, pools[0][2])
    for _ in range(2):
        da, dg = bank.poll(wait=True), group.poll(wait=True)
        for k in ("batch_index", "first_frame", "n_frames", "runes_dropped", "edges_dropped"):
            assert da[k] == dg[k], k
        for k in ("chunks", "peaks", "listeners", "edges", "runes", "rune_frames"):
            assert da[k].tobytes() == dg[k].tobytes(), k
    L = group._L
    arr = (C.c_void_p * 2)(ts[0].data_ptr(), None)
    assert L.sdr_group_process_device_iq8(group._h, arr, frames, fmt) == c.ERR_BAD_ARG
    arr = (C.c_void_p * 2)(ts[0].data_ptr(), ts[1].data_ptr() + 4)
    assert L.sdr_group_process_device_iq8(group._h, arr, frames, fmt) == c.ERR_BAD_ARG
    arr = (C.c_void_p * 2)(ts[0].data_ptr(), ts[1].data_ptr())
    assert L.sdr_group_process_device_iq8(group._h, arr, frames, 2) == c.ERR_BAD_ARG
    assert L.sdr_group_process_device_iq8(group._h, None, frames, fmt) == c.ERR_BAD_ARG
    assert L.sdr_group_push_iq8(group._h, bands, RATE[n], C.c_void_p(q.ctypes.data), 2 * n, fmt) == c.ERR_BAD_ARG
    assert L.sdr_group_push_iq8(group._h, 0, RATE[n], C.c_void_p(q.ctypes.data), 2 * n, -1) == c.ERR_BAD_ARG
    group.close()
    bank.close()


@both
def test_bad_arguments(capi, fmt):
    c = capi
    bank = c.Bank(RATE[1024], 1024, max_batch_frames=8)
    L = bank._L
    t = torch.zeros(9 * 2 * 1024 + 32, dtype=torch.uint8, device="cuda")
    ptr = C.c_void_p(t.data_ptr())
    assert L.sdr_process_device_iq8(None, ptr, 1, fmt) == c.ERR_BAD_ARG
    assert L.sdr_process_device_iq8(bank._h, None, 1, fmt) == c.ERR_BAD_ARG
    for off in (1, 2, 4, 8):
        assert L.sdr_process_device_iq8(bank._h, C.c_void_p(t.data_ptr() + off), 1, fmt) == c.ERR_BAD_ARG
    assert L.sdr_process_device_iq8(bank._h, ptr, 1, 2) == c.ERR_BAD_ARG
    assert L.sdr_process_device_iq8(bank._h, ptr, 1, -1) == c.ERR_BAD_ARG
    assert L.sdr_process_device_iq8(bank._h, ptr, 9, fmt) == c.ERR_BAD_ARG  # > max_batch_frames
    assert L.sdr_process_device_iq8(bank._h, ptr, 0, fmt) == c.OK
    assert L.sdr_process_device_stream_iq8(bank._h, ptr, 1, 1024, 2) == c.ERR_BAD_ARG
    assert L.sdr_process_device_stream_iq8(bank._h, None, 1, 1024, fmt) == c.ERR_BAD_ARG
    assert L.sdr_process_device_stream_iq8(bank._h, C.c_void_p(t.data_ptr() + 8), 1, 1024, fmt) == c.ERR_BAD_ARG
    assert L.sdr_graph_launch_iq8(bank._h, None, fmt) == c.ERR_BAD_ARG
    assert L.sdr_graph_capture_iq8(bank._h, 9, fmt) == c.ERR_BAD_ARG
    assert L.sdr_graph_capture_iq8(bank._h, 8, -1) == c.ERR_BAD_ARG
    arr = (C.c_void_p * bank.graph_batches)(*([t.data_ptr()] * bank.graph_batches))
    assert L.sdr_graph_launch_iq8(bank._h, arr, fmt) == c.ERR_STATE  # nothing captured
    bank.close()
    hopped = c.Bank(RATE[1024], 1024, max_batch_frames=8, hop=256)
    assert L.sdr_process_device_iq8(hopped._h, ptr, 1, fmt) == c.ERR_STATE  # the dense call on a bank with a hop
    assert L.sdr_graph_capture_iq8(hopped._h, 8, fmt) == c.ERR_STATE
    hopped.close()


@both
def test_rows_and_reports(capi, fmt):
    """Waterfall rows and listener reports on, N = 1024 over 250 frames: both blocks equal between the float32 bank and the
    8-bit one (they are format-blind; this pins it)."""
    n, tones, frames = 1024, 6, 250
    p = Pair(capi, n, 1, frames, tones, fmt)
    for bk in (p.a, p.b):
        bk.enable_rows(64)
        bk.enable_reports(True)
    q, bins, want = pool(n, tones, 950, fmt)
    p.attach([bins])
    x = batch(q, frames)[None]
    ta, tb = torch.from_numpy(to_f32(x, fmt)).cuda(), torch.from_numpy(np.ascontiguousarray(x)).cuda()
    torch.cuda.synchronize()
    p.a.process_device(ta.data_ptr(), frames)
    p.b.process_device_iq8(tb.data_ptr(), frames, fmt)
    p.sync()
    ra, rb = p.a.poll_rows(wait=True), p.b.poll_rows(wait=True)
    assert ra[0] == rb[0] and ra[1].shape == rb[1].shape == (2, 64) and ra[1].tobytes() == rb[1].tobytes()
    assert np.all(np.isfinite(ra[1]))
    pa, pb = p.a.poll_reports(wait=True), p.b.poll_reports(wait=True)
    assert pa[0] == pb[0] and len(pa[1]) > 0 and pa[1].tobytes() == pb[1].tobytes()
    assert p.check(frames) == 1
    check_oracle(p.b, 0, frames, want)
    p.close()
