"""A window on the frames (sdr_set_window, include/sdrainer_hip.h) on the GPU, bit for bit against the CPU oracle.

The specification is one line: the reference fed frame f, sample i = float32(x[i] * w[i]), real and imaginary part each.
So the oracle side of every comparison here is the oracle AS IT STANDS fed with the materialised frames multiplied by numpy
in float32 (parity_tools.windowed); everything the bank delivers and keeps must be the oracle's bits.  The tables of the
parity tests are random and asymmetric (0.25 - 1): a Hann table is symmetric and positive and would let a reversed or
shifted index through.  The driver is parity_case.Case with a window per batch; the hop-timed decoders are
parity_tools.decode's."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from parity_case import Case
from parity_tools import (DEMO, GEOMETRY, GROUP_BANDS as BANDS, GROUP_CENTER as CENTER, RATES as RATE, REC_FIELDS, Pair, assert_records_equal,  # noqa: F401
                          bits_equal, capi, check_batch_polled, check_demo_oracle, check_device_batch, decode, demo_oracle, demo_stream,
                          environment, frames_of, group_bands, make_stream, random_window, run_oracle, windowed)
from sdrainer_amd import synth

pytestmark = pytest.mark.gpu


# 1. Every input path ---------------------------------------------------------------------------------------------------
# test_overlap_gpu's rows (every kernel family windowed and strided: k_fft_psd one frame per workgroup at four sizes,
# k_fft_psd<14> at 256 frames and at 1024 and 2048 frames where k_fft_r32 would have run - the last with 256 listeners, whose
# refinement reads psd columns instead of the wide tap - and k_fft2p_a at both its sizes), two dense rows (hop = 0), and
# one row with SDR_FFT_FPW = 4 for the multi-frame workgroup (1100 frames: 275 workgroups, so the launcher keeps four).
ROWS = [g + (0,) for g in GEOMETRY] + [
    (512, 0, (300, 130), 1, 6, 12, 0),
    (8192, 0, (300, 130), 8, 16, 16, 0),
    (4096, 1024, (1100, 130), 1, 16, 24, 4),
]


def row_id(g):
    return f"N{g[0]}-hop{g[1]}-{g[2][0]}x{g[3]}-L{g[5]}" + (f"-fpw{g[6]}" if g[6] else "")


def row_run(g, sc16):
    n, hop, calls, n_bands, tones, listeners, _ = g
    seed = 7000 + n // 64 + hop // 32
    return Case.of_streams(n, hop, calls, n_bands, tones, listeners, sc16, seed, [random_window(n, seed + 1)] * len(calls))


@pytest.mark.parametrize("sc16", [False, True], ids=["f32", "sc16"])
@pytest.mark.parametrize("g", ROWS, ids=[row_id(g) for g in ROWS])
def test_every_input_path(capi, g, sc16):
    run = row_run(g, sc16)
    edges, peaks = run.oracle_counts()
    assert edges > 0 and peaks > 0, "the row's input shows the oracle no edge or no peak"
    with environment(**({"SDR_FFT_FPW": g[6]} if g[6] else {})):
        run.run(capi, min_edges=0).close()


# 2. All ones is no window ----------------------------------------------------------------------------------------------
def _snapshot(bank, res, n_bands, L, frames):
    """Everything a batch delivered and left, as bytes."""
    out = [(k, v.tobytes() if isinstance(v, np.ndarray) else v) for k, v in sorted(res.items())]
    for b in range(n_bands):
        out.append(bank.read_frame_records(b).tobytes())
        for f in sorted({0, frames // 2, frames - 1}):
            out += [x.tobytes() for x in bank.read_spectrum(b, f)]
        for lid in range(L):
            out += [x.tobytes() for x in bank.read_trace(b, lid)]
            out.append(bank.read_decoder_state(b, lid).tobytes())
    return out


# one N per kernel family: (N, hop, calls, bands, tones, listeners, SDR_FFT_FPW)
ONES = [
    (4096, 1024, (300, 130), 2, 8, 8, 0),     # k_fft_psd, one frame per workgroup
    (4096, 0, (1100, 130), 1, 8, 8, 4),       # k_fft_psd, four frames per workgroup
    (16384, 4096, (1024, 130), 1, 16, 16, 0),  # without a window k_fft_r32 and its wide tap, with one k_fft_psd<14>
    (65536, 8192, (160, 130), 1, 8, 8, 0),    # k_fft2p_a
]


@pytest.mark.parametrize("sc16", [False, True], ids=["f32", "sc16"])
@pytest.mark.parametrize("g", ONES, ids=[row_id(g) for g in ONES])
def test_all_ones_is_no_window(capi, g, sc16):
    """A table of 1.0f through the windowed kernels gives the bytes of a bank that never had a window, and so does a bank
    whose window was set and removed again."""
    import torch

    n, hop, calls, n_bands, tones, L, fpw = g
    step, rate, edge = hop or n, RATE[n], synth.default_edge_width(n)
    made = [make_stream(n, step, sum(calls), rate, tones, 8100 + n // 64 + 17 * b, sc16) for b in range(n_bands)]
    host = np.stack([m[1] if sc16 else m[0] for m in made])
    dev = torch.from_numpy(host).cuda()
    samples = host.shape[1]
    got = {}
    for mode in ("never", "ones", "removed"):
        with environment(**({"SDR_FFT_FPW": fpw} if fpw else {})):
            bank = capi.Bank(rate, n, n_bands=n_bands, edge_width=edge, max_batch_frames=max(calls), max_listeners=L, max_peaks=1024,
                             trace=True, hop=hop)
        bank.set_stream(torch.cuda.current_stream().cuda_stream)
        for b in range(n_bands):
            for bn in made[b][2][:L]:
                bank.attach(b, int(bn))
        bank.enable_results(True)
        if mode == "ones":
            bank.set_window(np.ones(n, np.float32))
        elif mode == "removed":
            bank.set_window(random_window(n, 5))
            bank.set_window(None)
        per, pos = [], 0
        for frames in calls:
            if hop:
                (bank.process_device_stream_sc16 if sc16 else bank.process_device_stream)(dev.data_ptr() + pos * step * 2 * dev.element_size(), frames, samples)
            else:
                batch = dev[:, pos * n:(pos + frames) * n].contiguous()
                (bank.process_device_sc16 if sc16 else bank.process_device)(batch.data_ptr(), frames)
            res = bank.poll(wait=True)
            per.append(_snapshot(bank, res, n_bands, L, frames))
            pos += frames
        assert sum(len(res[k]) for k in ("runes", "edges", "peaks")) > 0
        got[mode] = per
        bank.close()
    assert got["ones"] == got["never"], "a window of ones changes something"
    assert got["removed"] == got["never"], "a window set and removed leaves something behind"


# 3. Between batches ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc16", [False, True], ids=["f32", "sc16"])
def test_window_changes_between_batches(capi, sc16):
    """One stream in three calls, the window changed between them (none -> random -> Hann): the oracle fed the three frame
    ranges multiplied accordingly; rolling means, the open cumulation (250, 130 and 170 frames) and the decoders carry across."""
    n, hop = 4096, 1024
    run = Case.of_streams(n, hop, (250, 130, 170), 2, 12, 16, sc16, 8300, [None, random_window(n, 8301), synth.hann(n)])
    edges, peaks = run.oracle_counts()
    assert edges > 0 and peaks > 0
    run.run(capi, min_edges=0).close()


# 4. Staged, Kiwi, group, graph -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sc16", [False, True], ids=["f32", "sc16"])
def test_staged_pushes_with_a_hop(capi, sc16):
    """sdr_push_iq / sdr_push_iq_sc16 in pieces of odd numbers of hops, hop < N: the staged path reaches the same kernels."""
    n, hop, rate, frames, L, edge = 512, 128, 48_000, 437, 5, 70
    s, q, carriers = make_stream(n, hop, frames, rate, 4, seed=8400, sc16=sc16)
    bins = carriers + [carriers[0] + 1]
    w = random_window(n, 8401)
    ref = orc.Receiver(rate, n, edge)
    for b in bins:
        ref.attach(int(b))
    out = ref.process(windowed(frames_of(s, n, hop), w, n))
    decs = [decode(out["deb"][:, lid], rate, hop) for lid in range(L)]
    bank = capi.Bank(rate, n, edge_width=edge, max_batch_frames=512, max_listeners=8, max_peaks=64, hop=hop)
    assert [bank.attach(0, int(b)) for b in bins] == list(range(L))
    bank.set_window(w)
    host, push = (q if sc16 else s), (bank.push_iq_sc16 if sc16 else bank.push_iq)
    total_hops, pushed, at, i = host.shape[0] // hop, 0, 0, 0
    recs, debs, text = [], [[] for _ in range(L)], ["" for _ in range(L)]
    sizes = (1, 3, 7, 41, 5, 9, 63)
    while pushed < total_hops or bank.staged_frames(0) > 0:
        k = min(sizes[i % len(sizes)], total_hops - pushed)
        if k > 0:
            assert push(0, rate, host[pushed * hop:(pushed + k) * hop].reshape(-1)) == capi.OK
            pushed += k
        got = bank.process_staged()
        if got:
            recs.append(bank.read_frame_records(0))
            for lid in range(L):
                debs[lid].append(bank.read_keying_bits(0, lid))
                text[lid] += bank.read_text(0, lid)
            at += got
        i += 1
    assert at == frames
    recs = np.concatenate(recs)
    for f in REC_FIELDS:
        assert bits_equal(recs[f], out["frames"][f]), f
    for lid in range(L):
        assert np.array_equal(np.concatenate(debs[lid]), out["deb"][:, lid])
        assert text[lid] == decs[lid][0] and np.array_equal(bank.read_decoder_state(0, lid), decs[lid][1])
    assert any(text) and np.count_nonzero(np.diff(out["deb"].astype(np.int8), axis=0)) > 0
    bank.close()


def test_kiwi_payloads(capi):
    """sdr_push_kiwi_snd (dense; big-endian int16 unpacked on the device to float32): the window multiplies the unpacked
    values, what the reference's decodeIQBytes hands on times w."""
    n, rate, frames = 512, 12000, 120
    rng = np.random.default_rng(8500)
    iq16 = rng.integers(-3000, 3000, size=(frames, 2 * n)).astype(np.int16)
    tone = 12000 * np.exp(2j * np.pi * 40 * np.arange(n) / n)
    iq16[:, 0::2] += tone.real.astype(np.int16)
    iq16[:, 1::2] += tone.imag.astype(np.int16)
    w = random_window(n, 8501)
    bank = capi.Bank(rate, n, max_batch_frames=128, max_listeners=2, trace=True)
    ref = orc.Receiver(rate, n, 70)
    b = (40 + n // 2) % n
    bank.attach(0, b)
    ref.attach(b)
    bank.set_window(w)
    ref_iq, f = [], 0
    for k in [1, 2, 5, 12, 40, 60]:
        payload = bytes([0x01] + [7] * 16) + iq16[f:f + k].astype(">i2").tobytes()
        assert bank.push_kiwi_snd(0, rate, payload) == capi.OK
        ref_iq.append(orc.decode_iq_message(payload).reshape(k, 2 * n))
        f += k
    assert bank.process_staged() == frames
    out = ref.process(windowed(np.concatenate(ref_iq), w, n), want_spectrum=True)
    for fr in (0, 57, frames - 1):
        sp, psd = bank.read_spectrum(0, fr)
        assert bits_equal(sp, out["spectrum"][fr]) and bits_equal(psd, out["psd"][fr])
    recs = bank.read_frame_records(0)
    for fld in REC_FIELDS:
        assert bits_equal(recs[fld], out["frames"][fld]), fld
    v, raw, deb = bank.read_trace(0, 0)
    assert bits_equal(v, out["values"][:, 0].copy()) and np.array_equal(raw, out["raw"][:, 0]) and np.array_equal(deb, out["deb"][:, 0])
    assert np.array_equal(bank.read_keying_bits(0, 0), out["deb"][:, 0])
    bank.close()


def test_group_window(capi):
    """A two-member group on one GPU through sdr_group_set_window against ONE bank with the same window (every merged
    delivery equal, field by field), one band of each member against the oracle; the window changes between the batches
    (random -> none -> Hann), for every member at the same frame."""
    n, rate, tones, batches = 1024, 96000, 4, (250, 150, 200)
    edge = synth.default_edge_width(n)
    iq, bins = group_bands(sum(batches), rate, n, tones, seed=8600)
    p = Pair(capi, (0, 0), rate, n, edge_width=edge, max_listeners=8, max_batch_frames=max(batches), max_peaks=64)
    p.bank.enable_results(True)
    p.group.enable_results(True)
    watched = (2, 3)  # member 0 and member 1
    refs = {b: orc.Receiver(rate, n, edge, 15.0, 1, center_frequency=CENTER[b]) for b in watched}
    for b in range(BANDS):
        for t in bins[b]:
            p.attach(b, t)
            if b in refs:
                refs[b].attach(int(t))
    windows = [random_window(n, 8601), None, synth.hann(n)]
    f0, delivered = 0, 0
    for k, nf in enumerate(batches):
        p.bank.set_window(windows[k])
        p.group.set_window(windows[k])
        seg = iq[:, f0:f0 + nf]
        p.process(seg)
        res = p.polls()  # (asserts group == bank)
        assert res["batch_index"] == k and res["n_frames"] == nf
        delivered += len(res["edges"]) + len(res["peaks"])
        for b in watched:
            want = refs[b].process(seg[b] if windows[k] is None else windowed(seg[b], windows[k], n), want_spectrum=True)
            m, lb = p.group.member(b)
            assert_records_equal(m.read_frame_records(lb), want["frames"], f"band {b} (group)")
            assert_records_equal(p.bank.read_frame_records(b), want["frames"], f"band {b} (bank)")
            _, psd = m.read_spectrum(lb, nf - 1)
            assert bits_equal(psd, want["psd"][-1])
            for lid in range(tones):
                assert np.array_equal(m.read_keying_bits(lb, lid), want["deb"][:, lid])
        f0 += nf
    assert delivered > 0
    # the statuses reach the caller through the group as well
    L = capi.load()
    assert L.sdr_group_set_window(p.group._h, np.ones(n - 1, np.float32).ctypes.data_as(C.POINTER(C.c_float)), n - 1) == capi.ERR_BAD_ARG
    assert len(L.sdr_last_error()) > 0
    assert L.sdr_group_set_window(p.group._h, None, n) == capi.ERR_BAD_ARG
    p.close()


def test_graph_capture_with_a_window(capi):
    """sdr_graph_capture + two replays at config 5's geometry (8 bands, N = 8192, float32) with a window set before the
    capture: the capture records the windowed kernels and the table, the replays run with them."""
    import torch

    rate, n, tones, n_bands, per = 2_000_000, 8192, 16, 8, 230
    edge = synth.default_edge_width(n)
    w = random_window(n, 8700)
    bank = capi.Bank(rate, n, n_bands=n_bands, edge_width=edge, max_batch_frames=per, max_listeners=tones, max_peaks=256)
    K = bank.graph_batches
    total = 2 * K * per
    dev_iq, bins_per_band, host_iq = [], [], []
    for b in range(n_bands):
        iq, bins, _ = synth.make_band_torch(total, rate, n, tones, seed=8710 + 17 * b, device="cuda")
        dev_iq.append(iq)
        bins_per_band.append(bins)
        host_iq.append(windowed(iq.cpu().numpy(), w, n))
    centers = [7000000 + 50000 * b for b in range(n_bands)]
    refs, outs, _ = run_oracle(rate, n, edge, bins_per_band, host_iq, centers)
    stream = torch.cuda.Stream()
    bank.set_stream(stream.cuda_stream)
    for b in range(n_bands):
        bank.set_center_frequency(b, centers[b])
        for i, bn in enumerate(bins_per_band[b]):
            assert bank.attach(b, int(bn)) == i
    bank.enable_results(True)
    bank.set_window(w)
    bank.graph_capture(per)
    batches = [torch.stack([iq[k * per:(k + 1) * per] for iq in dev_iq]).contiguous() for k in range(2 * K)]
    torch.cuda.synchronize()
    text = [["" for _ in range(tones)] for _ in range(n_bands)]
    delivered = edges = peaks = 0
    for rep in range(2):
        bank.graph_launch([batches[rep * K + k].data_ptr() for k in range(K)])
        for k in range(K):
            res = bank.poll(wait=True)
            a = (rep * K + k) * per
            assert res["batch_index"] == delivered
            ne, npk = check_batch_polled(res, outs, a, a + per, tones, text, n_bands)
            edges, peaks, delivered = edges + ne, peaks + npk, delivered + 1
    bank.sync()
    assert bank.total_frames == total and edges > 0 and peaks > 0
    for b in range(n_bands):
        recs = bank.read_frame_records(b)
        for f in REC_FIELDS:
            assert bits_equal(recs[f], outs[b]["frames"][f][total - per:].copy()), f"band {b} field {f}"
        for lid in range(tones):
            assert text[b][lid] == refs[b].text(lid), f"band {b} listener {lid}"
            assert np.array_equal(bank.read_keying_bits(b, lid), outs[b]["deb"][total - per:, lid])
            assert np.array_equal(bank.read_decoder_state(b, lid), refs[b].decoder_state(lid))
    bank.close()


# 5. Statuses -----------------------------------------------------------------------------------------------------------
def test_statuses(capi):
    """Wrong n, a null table with n != 0, the listen half of a deferred batch pending, a graph captured: each its status and
    a message in sdr_last_error, and the bank works afterwards (with the window it had)."""
    import torch

    L = capi.load()
    n, rate, frames, edge = 4096, 192_000, 200, synth.default_edge_width(4096)
    fp = C.POINTER(C.c_float)

    def refused(code, bank, table, count):
        rc = L.sdr_set_window(bank._h, None if table is None else table.ctypes.data_as(fp), count)
        assert rc == code, (rc, L.sdr_last_error())
        assert len(L.sdr_last_error()) > 0

    iq, bins, _ = synth.make_band(2 * frames, rate, n, 8, seed=8800, free_last_window=True)
    w = random_window(n, 8801)
    ref = orc.Receiver(rate, n, edge)
    for b in bins:
        ref.attach(int(b))
    out = ref.process(windowed(iq, w, n))
    dev = torch.from_numpy(iq).cuda()
    bank = capi.Bank(rate, n, edge_width=edge, max_batch_frames=frames, max_listeners=8)
    bank.set_stream(torch.cuda.current_stream().cuda_stream)
    for b in bins:
        bank.attach(0, int(b))
    big = np.ones(2 * n, np.float32)
    refused(capi.ERR_BAD_ARG, bank, big, n - 1)
    refused(capi.ERR_BAD_ARG, bank, big, n + 1)
    refused(capi.ERR_BAD_ARG, bank, big, 2 * n)
    refused(capi.ERR_BAD_ARG, bank, big, 0)
    refused(capi.ERR_BAD_ARG, bank, None, n)
    assert L.sdr_set_window(None, big.ctypes.data_as(fp), n) == capi.ERR_BAD_ARG
    assert L.sdr_set_window(bank._h, None, 0) == capi.OK  # removing a window that was never set
    bank.set_window(w)
    # the listen half of a deferred batch is pending
    bank.enable_results(True)
    bank.defer_listen(True)
    bank.process_device(dev.data_ptr(), frames)
    bank.poll_peaks(wait=True)
    assert bank.listen_pending
    refused(capi.ERR_STATE, bank, np.ones(n, np.float32), n)
    refused(capi.ERR_STATE, bank, None, 0)
    bank.process_listen()
    bank.poll(wait=True)
    bank.defer_listen(False)
    # ... and the refused calls changed nothing: the second batch still runs with w
    bank.process_device(dev[frames:].data_ptr(), frames)
    bank.poll(wait=True)
    check_device_batch(bank, [out], frames, 2 * frames, 1, [range(8)], 1)
    bank.set_window(None)
    bank.set_window(synth.hann(n))
    bank.close()
    # a graph is captured (a fresh bank: a capture starts at a multiple of sdr_graph_batches() batches)
    bank = capi.Bank(rate, n, edge_width=edge, max_batch_frames=frames, max_listeners=8)
    bank.set_stream(torch.cuda.Stream().cuda_stream)
    for b in bins:
        bank.attach(0, int(b))
    bank.set_window(w)
    bank.graph_capture(frames)
    refused(capi.ERR_STATE, bank, np.ones(n, np.float32), n)
    refused(capi.ERR_STATE, bank, None, 0)
    bank.graph_release()
    bank.set_window(w)  # (accepted again once the capture is gone)
    bank.process_device(dev.data_ptr(), frames)
    bank.sync()
    check_device_batch(bank, [out], 0, frames, 1, [range(8)], 0)
    bank.close()


# 6. The case the feature exists for ------------------------------------------------------------------------------------
@pytest.mark.parametrize("neighbour", ["carrier", "soft"])
def test_a_strong_neighbour_needs_the_window(capi, neighbour):
    """test_window_host's demonstration on the GPU.  Measured with the oracle over the stream's 72 cumulations, rectangular /
    Hann: 'dl1abc' read 0 / 6 times (unkeyed neighbour) and 0 / 5 times (soft-keyed); the two stations one peak run in 72 / 0
    and 63 / 0 cumulations; longest run 346 / 12 and 231 / 12 bins.  The assertions on the oracle come first; then the
    bank's keying bits, text, decoder state and peak lists equal the oracle's under both windows."""
    import torch

    d = DEMO
    rate, n, hop = d["rate"], d["n"], d["hop"]
    s = demo_stream(neighbour)
    want = {"rectangular": demo_oracle(s, None), "hann": demo_oracle(s, synth.hann(n))}
    check_demo_oracle(want["rectangular"], want["hann"])
    dev = torch.from_numpy(s).cuda()
    for name, w in (("rectangular", None), ("hann", synth.hann(n))):
        o = want[name]
        per = 1200
        bank = capi.Bank(rate, n, edge_width=d["edge"], max_batch_frames=per, max_listeners=1, max_peaks=1024, find_peaks=True, hop=hop)
        bank.set_stream(torch.cuda.current_stream().cuda_stream)
        assert bank.attach(0, d["bin"]) == 0
        if w is not None:
            bank.set_window(w)
        text, deb, peak_frames, peaks = "", [], [], []
        for a in range(0, o["frames"], per):
            k = min(per, o["frames"] - a)
            bank.process_device_stream(dev.data_ptr() + a * hop * 8, k, (k - 1) * hop + n)
            deb.append(bank.read_keying_bits(0, 0))
            text += bank.read_text(0, 0)
            for c in range(bank.last_batch_chunks):
                pk, _, fr = bank.read_peaks(0, c)
                peak_frames.append(a + fr)
                peaks.append(pk)
        assert np.array_equal(np.concatenate(deb), o["deb"]), f"{name}: keying bits"
        assert text == o["text"], f"{name}: {text!r} != {o['text']!r}"
        assert np.array_equal(bank.read_decoder_state(0, 0), o["state"]), f"{name}: decoder state"
        assert peak_frames == o["peak_frames"] and peaks == o["peaks"], f"{name}: peak lists"
        bank.close()
