"""Block sizes 32768 and 65536 (k_fft_2p.hip: the two-phase FFT; the chains' noise floor; k_find_peaks_wide) on the GPU,
against the CPU oracle bit for bit: frame records, keying bits and edges, decoded text and decoder state, every completed
cumulation, and the peak lists with their frequencies as sdr_poll delivers them (tests/test_gpu_parity_bench_sizes.py's
checks).  One band and three, 256 listeners, two batches that cross cumulation boundaries and a short batch behind them
whose length divides no frame group; the same with each alternative path forced, in child processes; sc16 input against
float32, eagerly and as graph replays; float32 graph replays; staged float32 and KiwiSDR input against device input; a
two-member group against one bank; listeners bound inside a deferred batch."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as orc
from parity_case import Case
from parity_tools import REC_FIELDS, bits_equal, capi, check_batch_polled, run_oracle  # noqa: F401 (capi: the fixture)
from sdrainer_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# config 3's bin width at both sizes is 61 Hz: 2 MS/s at 32768 points, 4 MS/s at 65536
RATE = {32768: 2_000_000, 65536: 4_000_000}
FRAMES = {32768: 1024, 65536: 512}  # per batch; two of them, then a shorter batch


@pytest.mark.parametrize("n", [32768, 65536])
def test_wide_block_one_band(capi, n):
    Case(n, 1, 256, 256, [("batch", FRAMES[n])] * 2 + [("batch", 333)], seed=7000 + n % 1000, rate=RATE[n]).run(capi).close()


@pytest.mark.parametrize("n", [32768, 65536])
def test_wide_block_three_bands(capi, n):
    Case(n, 3, 256, 256, [("batch", FRAMES[n] // 2)] * 2 + [("batch", 211)], seed=7100 + n % 1000, rate=RATE[n]).run(capi).close()


@pytest.mark.parametrize("env", [{"SDR_CUM_BOUND": "0"}, {"SDR_CUM_BOUND": "1"}, {"SDR_CUM_BOUND": "1", "SDR_REFINE_WIDE": "0"},
                                 {"SDR_CUM_BOUND": "1", "SDR_REFINE_WIDE": "1"}, {"SDR_NOISE_PATH": "chains"},
                                 {"SDR_FFT2P_GROUP_MB": "0"}, {"SDR_FFT2P_GROUP_MB": "1"}],
                         ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_wide_block_forced_paths(env):
    """The one-band case with one path forced (the switches are read when a bank is created: a fresh process each)."""
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_block_size_wide_gpu.py"), "-q", "-x", "-m", "gpu",
                        "-k", "test_wide_block_one_band", "-p", "no:cacheprovider"], env=dict(os.environ, **env), cwd=ROOT,
                       capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr[-2000:]
    assert "2 passed" in p.stdout, p.stdout[-2000:]


def _quantised(n, frames, tones, seed):
    iq, bins, _ = synth.make_band(frames, RATE[n], n, tones, seed=seed)
    q = np.clip(np.rint(iq.astype(np.float64) * 3.0e5), -32768, 32767).astype(np.int16)
    q[:, :6] = np.array([32767, -32768, -32767, 0, 1, -1], np.int16)
    return q, bins


def _same_outputs(a, b, bands, frames):
    for band in range(bands):
        for f in range(frames):
            sa, pa = a.read_spectrum(band, f)
            sb, pb = b.read_spectrum(band, f)
            assert pa.tobytes() == pb.tobytes() and sa.tobytes() == sb.tobytes(), f"band {band} frame {f}"
        assert a.read_frame_records(band).tobytes() == b.read_frame_records(band).tobytes(), f"band {band}: frame records"
    n = 0
    while True:
        da, db = a.poll(wait=False), b.poll(wait=False)
        assert (da is None) == (db is None)
        if da is None:
            break
        for k in ("chunks", "peaks", "listeners", "edges", "runes", "rune_frames"):
            assert da[k].tobytes() == db[k].tobytes(), k
        n += 1
    return n


@pytest.mark.parametrize("n", [32768, 65536])
def test_wide_block_sc16_equals_float32_and_oracle(capi, n):
    """sc16 frames through k_fft2p_a<SC16> give what float32(x) / 32767 gives through the float32 path; the psd rows
    equal the oracle's."""
    import torch

    frames, tones = 250, 32
    q, bins = _quantised(n, frames, tones, seed=8000 + n % 1000)
    f32 = q.astype(np.float32) / np.float32(32767.0)
    a = capi.Bank(RATE[n], n, max_batch_frames=frames, max_listeners=tones)
    b = capi.Bank(RATE[n], n, max_batch_frames=frames, max_listeners=tones)
    for bk in (a, b):
        bk.enable_results(True)
        for bn in bins:
            bk.attach(0, int(bn))
    ta, tb = torch.from_numpy(f32).cuda(), torch.from_numpy(q).cuda()
    torch.cuda.synchronize()
    a.process_device(ta.data_ptr(), frames)
    b.process_device_sc16(tb.data_ptr(), frames)
    a.sync()
    b.sync()
    assert _same_outputs(a, b, 1, frames) == 1
    for f in (0, 1, frames // 2, frames - 1):
        _, want = orc.iq_to_spectrum_and_psd(f32[f])
        _, got = b.read_spectrum(0, f)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"frame {f}: psd differs from the oracle"
    a.close()
    b.close()


@pytest.mark.parametrize("n", [32768, 65536])
def test_wide_block_staged_equals_device(capi, n):
    """sdr_push_iq -> sdr_process_staged gives what process_device gives."""
    import torch

    frames, tones = 230, 16
    iq, bins, _ = synth.make_band(frames, RATE[n], n, tones, seed=8100 + n % 1000)
    a = capi.Bank(RATE[n], n, max_batch_frames=frames, max_listeners=tones)
    b = capi.Bank(RATE[n], n, max_batch_frames=frames, max_listeners=tones)
    for bk in (a, b):
        bk.enable_results(True)
        for bn in bins:
            bk.attach(0, int(bn))
    t = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    a.process_device(t.data_ptr(), frames)
    b.push_iq(0, RATE[n], iq.reshape(-1))
    assert b.process_staged() == frames
    a.sync()
    b.sync()
    assert _same_outputs(a, b, 1, frames) == 1
    a.close()
    b.close()


@pytest.mark.parametrize("n", [32768, 65536])
def test_wide_block_graph_mode(capi, n):
    """hipGraph replays (float32): two replays of sdr_graph_batches() batches against the oracle."""
    import torch

    rate, tones, n_bands, per = RATE[n], 64, 1, 130
    edge = synth.default_edge_width(n)
    bank = capi.Bank(rate, n, n_bands=n_bands, edge_width=edge, max_batch_frames=per, max_listeners=tones, max_peaks=1024)
    K = bank.graph_batches
    total = 2 * K * per
    iq, bins, _ = synth.make_band_torch(total, rate, n, tones, seed=8200 + n % 1000, device="cuda")
    refs, outs, _ = run_oracle(rate, n, edge, [bins], [iq.cpu().numpy()], [14000000])
    stream = torch.cuda.Stream()
    bank.set_stream(stream.cuda_stream)
    bank.set_center_frequency(0, 14000000)
    for i, bn in enumerate(bins):
        assert bank.attach(0, int(bn)) == i
    bank.enable_results(True)
    bank.graph_capture(per)
    batches = [iq[k * per:(k + 1) * per].contiguous() for k in range(2 * K)]
    torch.cuda.synchronize()
    text = [["" for _ in range(tones)]]
    delivered = 0
    for rep in range(2):
        bank.graph_launch([batches[rep * K + k].data_ptr() for k in range(K)])
        for k in range(K):
            res = bank.poll(wait=True)
            a = (rep * K + k) * per
            assert res["batch_index"] == delivered
            check_batch_polled(res, outs, a, a + per, tones, text, n_bands)
            delivered += 1
    bank.sync()
    recs = bank.read_frame_records(0)
    for f in REC_FIELDS:
        assert bits_equal(recs[f], outs[0]["frames"][f][total - per:].copy()), f"field {f}"
    for lid in range(tones):
        assert text[0][lid] == refs[0].text(lid), f"listener {lid}"
        assert np.array_equal(bank.read_decoder_state(0, lid), refs[0].decoder_state(lid))
    bank.close()


def _pair_banks(capi, n, frames, tones, bins, bands=1, **kw):
    banks = []
    for _ in range(2):
        bk = capi.Bank(RATE[n], n, n_bands=bands, max_batch_frames=frames, max_listeners=tones, **kw)
        bk.enable_results(True)
        for band in range(bands):
            for bn in bins[band]:
                bk.attach(band, int(bn))
        banks.append(bk)
    return banks


@pytest.mark.parametrize("n", [32768, 65536])
def test_wide_block_kiwi_staged_equals_device(capi, n):
    """KiwiSDR SND payloads (big-endian int16, unpacked on the device to float32) through sdr_push_kiwi_snd ->
    sdr_process_staged give what process_device gives on the decoded float32 frames; the psd rows equal the oracle's."""
    import torch

    frames, tones = 120, 16
    q, bins = _quantised(n, frames, tones, seed=8300 + n % 1000)
    a, b = _pair_banks(capi, n, frames, tones, [bins])
    ref_iq, f = [], 0
    for k in (1, 2, 5, 12, 40, 60):  # messages of several frames, as the websocket delivers them
        payload = bytes([0x01] + [7] * 16) + q[f:f + k].astype(">i2").tobytes()
        assert b.push_kiwi_snd(0, RATE[n], payload) == capi.OK
        ref_iq.append(orc.decode_iq_message(payload).reshape(k, 2 * n))
        f += k
    iq = np.ascontiguousarray(np.concatenate(ref_iq))
    t = torch.from_numpy(iq).cuda()
    torch.cuda.synchronize()
    a.process_device(t.data_ptr(), frames)
    assert b.process_staged() == frames
    a.sync()
    b.sync()
    assert _same_outputs(a, b, 1, frames) == 1
    for fr in (0, frames - 1):
        _, want = orc.iq_to_spectrum_and_psd(iq[fr])
        assert np.array_equal(b.read_spectrum(0, fr)[1].view(np.uint32), want.view(np.uint32)), f"frame {fr}"
    a.close()
    b.close()


@pytest.mark.parametrize("n", [32768, 65536])
def test_wide_block_graph_sc16_equals_float32(capi, n):
    """sdr_graph_capture_sc16 / _launch_sc16 (k_fft2p_a<SC16> reading the replay's cursors) against the float32 graph of
    the converted values, two replays; psd rows of the last batch equal the oracle's."""
    import torch

    frames, tones = 60, 16
    q, bins = _quantised(n, frames, tones, seed=8400 + n % 1000)
    a, b = _pair_banks(capi, n, frames, tones, [bins])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    a.set_stream(streams[0].cuda_stream)
    b.set_stream(streams[1].cuda_stream)
    K = a.graph_batches
    a.graph_capture(frames)
    b.graph_capture_sc16(frames)
    rng = np.random.default_rng(n)
    for rep in range(2):
        qs = [np.roll(q, int(rng.integers(1, frames)), axis=0) for _ in range(K)]  # a different batch each time
        ta = [torch.from_numpy(x.astype(np.float32) / np.float32(32767.0)).cuda() for x in qs]
        tb = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in qs]
        torch.cuda.synchronize()
        a.graph_launch([x.data_ptr() for x in ta])
        b.graph_launch_sc16([x.data_ptr() for x in tb])
        a.sync()
        b.sync()
        assert _same_outputs(a, b, 1, frames) == K
        last = qs[-1].astype(np.float32) / np.float32(32767.0)
        for fr in (0, frames - 1):
            _, want = orc.iq_to_spectrum_and_psd(last[fr])
            assert np.array_equal(b.read_spectrum(0, fr)[1].view(np.uint32), want.view(np.uint32)), f"replay {rep} frame {fr}"
    a.graph_release()
    b.graph_release()
    a.close()
    b.close()


@pytest.mark.parametrize("n", [32768, 65536])
def test_wide_block_group_equals_one_bank(capi, n):
    """A two-member sdr_group on device 0 (bands dealt over the members), fed by device pointers and by staged pushes,
    equals one bank of the same bands."""
    import torch

    frames, tones, bands = 110, 8, 2
    qs = [_quantised(n, frames, tones, seed=8500 + 7 * band + n % 1000) for band in range(bands)]
    iq = np.stack([x.astype(np.float32) / np.float32(32767.0) for x, _ in qs])
    bank = capi.Bank(RATE[n], n, n_bands=bands, max_batch_frames=frames, max_listeners=tones)
    group = capi.Group((0, 0), RATE[n], n, bands, max_batch_frames=frames, max_listeners=tones)
    bank.enable_results(True)
    group.enable_results(True)
    for band in range(bands):
        m, lb = group.member(band)
        for bn in qs[band][1]:
            assert bank.attach(band, int(bn)) == m.attach(lb, int(bn))
    t = torch.from_numpy(iq).cuda()
    ts = [torch.from_numpy(np.ascontiguousarray(iq[m::2])).cuda() for m in range(2)]
    torch.cuda.synchronize()
    bank.process_device(t.data_ptr(), frames)
    group.process_device([x.data_ptr() for x in ts], frames)
    for band in range(bands):
        assert bank.push_iq(band, RATE[n], iq[band]) == capi.OK
        assert group.push_iq(band, RATE[n], iq[band]) == capi.OK
    assert bank.process_staged() == group.process_staged() == frames
    bank.sync()
    group.sync()
    for band in range(bands):
        m, lb = group.member(band)
        for fr in (0, frames - 1):
            assert bank.read_spectrum(band, fr)[1].tobytes() == m.read_spectrum(lb, fr)[1].tobytes()
        assert bank.read_frame_records(band).tobytes() == m.read_frame_records(lb).tobytes()
    for _ in range(2):
        da, dg = bank.poll(wait=True), group.poll(wait=True)
        for k in ("batch_index", "first_frame", "n_frames", "runes_dropped", "edges_dropped"):
            assert da[k] == dg[k], k
        for k in ("chunks", "peaks", "listeners", "edges", "runes", "rune_frames"):
            assert da[k].tobytes() == dg[k].tobytes(), k
    group.close()
    bank.close()


@pytest.mark.parametrize("n", [32768, 65536])
def test_wide_block_listeners_bound_inside_a_batch(capi, n):
    """The deferred listen half: listeners bound with sdr_attach_at at cumulation boundaries INSIDE the batch (gathered
    from the retained psd rows, decoders starting mid-batch) beside listeners there from the start, against the oracle
    run cumulation by cumulation with a plain attach at every boundary."""
    import torch

    rate, frames, early, late = RATE[n], 400, 32, 3
    edge = synth.default_edge_width(n)
    iq, bins, _ = synth.make_band_torch(frames, rate, n, early + late, seed=8600 + n % 1000, device="cuda", free_last_window=True)
    host = iq.cpu().numpy()
    ref = orc.Receiver(rate, n, edge, 15.0, 1, center_frequency=14000000)
    for bn in bins[:early]:
        ref.attach(int(bn))
    starts, outs, pos = {}, [], 0
    for j in range(late):
        boundary = 100 * (j + 1)
        outs.append((pos, ref.process(host[pos:boundary])))
        pos = boundary
        starts[ref.attach(int(bins[early + j]))] = boundary
    outs.append((pos, ref.process(host[pos:])))

    bank = capi.Bank(rate, n, edge_width=edge, max_batch_frames=frames, max_listeners=early + late, max_peaks=1024)
    bank.set_stream(torch.cuda.current_stream().cuda_stream)
    bank.set_center_frequency(0, 14000000)
    for i, bn in enumerate(bins[:early]):
        assert bank.attach(0, int(bn)) == i
    bank.enable_results(True)
    bank.defer_listen(True)
    bank.process_device(iq.data_ptr(), frames)
    pk = bank.poll_peaks(wait=True)
    assert [int(c["frame"]) for c in pk["chunks"]] == list(range(99, frames, 100))
    for lid, s in sorted(starts.items()):
        assert bank.attach_at(0, int(bins[lid]), s) == lid
    bank.process_listen()
    res = bank.poll(wait=True)
    assert res["n_frames"] == frames and res["runes_dropped"] == 0 and res["edges_dropped"] == 0
    by = {int(r["listener"]): r for r in res["listeners"]}
    n_edges = 0
    for lid in range(early + late):
        s = starts.get(lid, 0)
        want, last = [], 0
        for base_frame, out in outs:
            if out["deb"].shape[1] <= lid or base_frame + out["deb"].shape[0] <= s:
                continue
            deb = out["deb"][:, lid].astype(np.int8)
            idx = np.flatnonzero(np.diff(np.concatenate([[last], deb])) != 0)
            want += [(base_frame + int(i), int(deb[i])) for i in idx if base_frame + i >= s]
            last = int(deb[-1])
        r = by.get(lid)
        got = [] if r is None else [(int(x["frame"]), int(x["state"])) for x in res["edges"][r["first_edge"]:r["first_edge"] + r["n_edges"]]]
        assert got == want, f"listener {lid} (from frame {s})"
        text = "" if r is None else "".join(chr(int(x)) for x in res["runes"][r["first_rune"]:r["first_rune"] + r["n_runes"]])
        assert text == ref.text(lid), f"listener {lid} text"
        assert np.array_equal(bank.read_decoder_state(0, lid), ref.decoder_state(lid)), f"listener {lid} state"
        n_edges += len(got)
    assert n_edges > 0
    bank.close()
