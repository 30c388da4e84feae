"""Overlapped frames on the GPU (sdr_config.hop < block_size; include/sdrainer_hip.h sdr_process_device_stream), bit for bit
against the CPU oracle fed with the materialised frames: frame f of a band is stream[f * hop : f * hop + N].

Inputs are continuous streams of keyed carriers over noise with one noise window left carrier-free
(parity_tools.make_stream); the driver is parity_case.Case with a hop.

What means time follows the hop: the listeners' decoder is cw.NewDecoder(sampleRate, hop).  The oracle's receiver builds
its decoders from the block size, so each listener's debounced bits from the oracle receiver go through
oracle.Decoder(sample_rate, hop); its text, 12-value state and the tick that wrote each rune are what the GPU must give.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from parity_case import Case
from parity_tools import (GEOMETRY, RATES as RATE, REC_FIELDS, bits_equal, capi, check_device_batch, decode, frames_of,  # noqa: F401
                          make_stream, run_oracle)
from sdrainer_amd import synth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("sc16", [False, True], ids=["f32", "sc16"])
@pytest.mark.parametrize("n,hop,calls,n_bands,tones,listeners", GEOMETRY, ids=[f"N{g[0]}-hop{g[1]}-{g[2][0]}x{g[3]}-L{g[5]}" for g in GEOMETRY])
def test_geometry(capi, n, hop, calls, n_bands, tones, listeners, sc16):
    Case.of_streams(n, hop, calls, n_bands, tones, listeners, sc16, seed=7000 + n // 64 + hop // 32).run(capi, min_edges=0).close()


def _collect(bank, n_bands, L):
    """What the last batch left: records, keying bits, text, peaks (by completing frame within the batch)."""
    out = []
    for b in range(n_bands):
        recs = bank.read_frame_records(b)
        debs = [bank.read_keying_bits(b, lid) for lid in range(L)]
        text = [bank.read_text(b, lid) for lid in range(L)]
        pk = [(bank.read_peaks(b, c)[2], bank.read_peaks(b, c)[0], bank.read_cumulation(b, c)) for c in range(bank.last_batch_chunks)]
        out.append((recs, debs, text, pk))
    return out


@pytest.mark.parametrize("sc16", [False, True], ids=["f32", "sc16"])
def test_split_invariance(capi, sc16):
    """One stream as one call; as calls of 1 / 99 / 100 / 101 / the rest through _stream (pointer advanced by frames * hop);
    and through sdr_push_iq(_sc16) in pieces of odd numbers of hops with sdr_process_staged_limit cuts: the same results and
    the same carried state, the oracle's."""
    import torch

    n, hop, rate, frames, L = 512, 128, 48_000, 437, 5
    s, q, carriers = make_stream(n, hop, frames, rate, 4, seed=99, sc16=sc16)
    bins = carriers + [carriers[0] + 1]
    _, (out,), (decs,) = run_oracle(rate, n, 70, [bins], [s], [0], hop)
    dev = torch.from_numpy(np.ascontiguousarray(q if sc16 else s)).cuda()
    size = dev.element_size()

    def bank_new():
        bank = capi.Bank(rate, n, edge_width=70, max_batch_frames=512, max_listeners=8, max_peaks=64, hop=hop)
        assert [bank.attach(0, int(b)) for b in bins] == list(range(L))
        return bank

    def check(bank, pieces):
        """pieces: per processed batch what _collect returned, in order."""
        recs = np.concatenate([p[0][0] for p in pieces])
        for f in REC_FIELDS:
            assert bits_equal(recs[f], out["frames"][f]), f
        at, peaks, cums = 0, [], []
        for p in pieces:
            peaks += [(at + fr, pk) for fr, pk, _ in p[0][3]]
            cums += [c for _, _, c in p[0][3]]
            at += len(p[0][0])
        assert at == frames
        assert [f for f, _ in peaks] == list(out["peak_frames"]) and [p for _, p in peaks] == out["peaks"]
        assert all(bits_equal(c, w) for c, w in zip(cums, out["cumulation"])) and len(cums) == len(out["cumulation"])
        for lid in range(L):
            assert np.array_equal(np.concatenate([p[0][1][lid] for p in pieces]), out["deb"][:, lid])
            assert "".join(p[0][2][lid] for p in pieces) == decs[lid][0]
            assert np.array_equal(bank.read_decoder_state(0, lid), decs[lid][1])
        assert bank.total_frames == frames
        bank.close()

    stream_call = lambda bank: bank.process_device_stream_sc16 if sc16 else bank.process_device_stream
    span = lambda k: (k - 1) * hop + n
    # one call
    bank = bank_new()
    stream_call(bank)(dev.data_ptr(), frames, span(frames))
    check(bank, [_collect(bank, 1, L)])
    # 1 / 99 / 100 / 101 / the rest
    bank, pos, pieces = bank_new(), 0, []
    for k in (1, 99, 100, 101, frames - 301):
        stream_call(bank)(dev.data_ptr() + pos * hop * 2 * size, k, span(k))
        pieces.append(_collect(bank, 1, L))
        pos += k
    check(bank, pieces)
    # staged: pieces of odd numbers of hops, cuts by sdr_process_staged_limit
    bank, pieces, at = bank_new(), [], 0
    host = q if sc16 else s
    push = bank.push_iq_sc16 if sc16 else bank.push_iq
    total_hops = host.shape[0] // hop
    sizes, limits = (1, 3, 7, 41, 5, 9, 63), (1000, 2, 1000, 7, 1, 1000, 30)
    assert bank.staged_frames(0) == 0
    i = pushed = 0
    while pushed < total_hops or bank.staged_frames(0) > 0:
        k = min(sizes[i % len(sizes)], total_hops - pushed)
        if k > 0:
            assert push(0, rate, host[pushed * hop:(pushed + k) * hop].reshape(-1)) == capi.OK
            pushed += k
        # complete frames: max(0, (history + staged - (N - hop)) / hop), the history N - hop samples once a batch has run
        assert bank.staged_frames(0) == max(0, pushed - at - (n // hop - 1))
        got = bank.process_staged_limit(limits[i % len(limits)])
        assert got == min(limits[i % len(limits)], max(0, pushed - at - (n // hop - 1)))
        if got:
            pieces.append(_collect(bank, 1, L))
            at += got
        i += 1
    assert len(pieces) > 10
    check(bank, pieces)


def test_staged_statuses(capi):
    n, hop, rate = 1024, 256, 48_000
    bank = capi.Bank(rate, n, max_batch_frames=8, max_listeners=1, hop=hop)
    x = np.zeros(2 * n * 4, np.float32)
    assert bank.push_iq(0, rate, x[:2 * hop - 2]) == capi.ERR_BAD_SIZE
    assert bank.push_iq(0, rate, x[:2 * (n - 1)]) == capi.ERR_BAD_SIZE
    assert bank.push_iq(0, rate + 1, x[:2 * hop]) == capi.ERR_BAD_RATE
    # capacity: (8 - 1) * 256 + 1024 = 2816 samples = 11 hops
    assert bank.push_iq(0, rate, x[:2 * hop * 11]) == capi.OK
    assert bank.staged_frames(0) == 8
    assert bank.push_iq(0, rate, x[:2 * hop]) == capi.ERR_WOULD_DROP
    assert bank.push_iq_sc16(0, rate, np.zeros(2 * hop, np.int16)) == capi.ERR_WOULD_DROP
    assert bank.process_staged() == 8
    # the history (3 hops) stays: 8 more hops are 8 more frames, a ninth would not fit
    assert bank.staged_frames(0) == 0
    assert bank.push_iq(0, rate, x[:2 * hop * 8]) == capi.OK and bank.staged_frames(0) == 8
    assert bank.push_iq(0, rate, x[:2 * hop]) == capi.ERR_WOULD_DROP
    bank.close()


@pytest.mark.parametrize("sc16", [False, True], ids=["f32", "sc16"])
@pytest.mark.parametrize("hop_arg", [0, 4096])
def test_hop_equal_block_size_is_process_device(capi, hop_arg, sc16):
    """hop = 0 and hop = block_size through _stream with the dense band stride: sdr_process_device on the same frames, what
    sdr_poll delivers included."""
    import torch

    n, rate, frames, n_bands, tones = 4096, 192_000, 300, 2, 8
    made = [synth.make_band(frames, rate, n, tones, seed=4100 + b, free_last_window=True) for b in range(n_bands)]
    host = np.stack([m[0] for m in made])
    if sc16:
        host = np.rint(host.astype(np.float64) * 3.0e4).astype(np.int16)
    dev = torch.from_numpy(host).cuda()
    got = []
    for stream in (False, True):
        bank = capi.Bank(rate, n, n_bands=n_bands, max_batch_frames=256, max_listeners=tones, trace=True, hop=hop_arg if stream else 0)
        assert bank.hop == n
        bank.set_stream(torch.cuda.current_stream().cuda_stream)
        for b in range(n_bands):
            for bn in made[b][1]:
                bank.attach(b, int(bn))
        bank.enable_results(True)
        per = []
        for a, e in ((0, 256), (256, 300)):
            batch = dev[:, a:e].contiguous()
            if stream:
                (bank.process_device_stream_sc16 if sc16 else bank.process_device_stream)(batch.data_ptr(), e - a, (e - a) * n)
            else:
                (bank.process_device_sc16 if sc16 else bank.process_device)(batch.data_ptr(), e - a)
            res = bank.poll(wait=True)
            per.append((res, [bank.read_frame_records(b) for b in range(n_bands)], [bank.read_spectrum(b, e - a - 1) for b in range(n_bands)],
                        [[bank.read_trace(b, lid) for lid in range(tones)] for b in range(n_bands)]))
        got.append((per, [[bank.read_decoder_state(b, lid) for lid in range(tones)] for b in range(n_bands)]))
        bank.close()
    (pa, sa), (pb, sb) = got
    for (ra, recs_a, sp_a, tr_a), (rb, recs_b, sp_b, tr_b) in zip(pa, pb):
        assert set(ra) == set(rb)
        for key in ra:
            if isinstance(ra[key], np.ndarray):
                assert ra[key].tobytes() == rb[key].tobytes(), key
            else:
                assert ra[key] == rb[key], key
        assert sum(len(r["runes"]) + len(r["edges"]) + len(r["peaks"]) for r in (ra,)) > 0
        assert all(x.tobytes() == y.tobytes() for x, y in zip(recs_a, recs_b))
        assert all(x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() for x, y in zip(sp_a, sp_b))
        assert all(u.tobytes() == v.tobytes() for ba, bb in zip(tr_a, tr_b) for x, y in zip(ba, bb) for u, v in zip(x, y))
    assert all(np.array_equal(x, y) for ba, bb in zip(sa, sb) for x, y in zip(ba, bb))


@pytest.mark.parametrize("sc16", [False, True], ids=["f32", "sc16"])
def test_band_stride_and_shared_buffer(capi, sc16):
    """A band stride larger than the dense one (padding behind every band's stream), and two bands whose streams are ONE
    buffer read at different offsets (band 1 starts stride samples into band 0's stream, not a whole number of hops): each
    band gives its own oracle's result."""
    import torch

    n, hop = 4096, 1024
    Case.of_streams(n, hop, (300, 130), 3, 8, 12, sc16, seed=5200, pad=52).run(capi, min_edges=0).close()
    rate, edge, frames = RATE[n], synth.default_edge_width(n), 200
    stride = (frames - 1) * hop + n + 36
    s, q, carriers = make_stream(n, hop, frames + (stride + hop - 1) // hop, rate, 8, seed=5300, sc16=sc16)
    streams = [s[:stride + 4000], s[stride:]]
    bins = [carriers, carriers]
    _, outs, decs = run_oracle(rate, n, edge, bins, [x[:(frames - 1) * hop + n] for x in streams], [0, 0], hop)
    dev = torch.from_numpy(np.ascontiguousarray(q if sc16 else s)).cuda()
    bank = capi.Bank(rate, n, n_bands=2, edge_width=edge, max_batch_frames=frames, max_listeners=8, hop=hop)
    bank.set_stream(torch.cuda.current_stream().cuda_stream)
    for b in range(2):
        for bn in carriers:
            bank.attach(b, int(bn))
    (bank.process_device_stream_sc16 if sc16 else bank.process_device_stream)(dev.data_ptr(), frames, stride)
    bank.sync()
    check_device_batch(bank, outs, 0, frames, 2, [range(8)] * 2, 0)
    for b in range(2):
        for lid in range(8):
            assert bank.read_text(b, lid) == decs[b][lid][0]
            assert np.array_equal(bank.read_decoder_state(b, lid), decs[b][lid][1])
    assert not np.array_equal(outs[0]["frames"]["min_mean"], outs[1]["frames"]["min_mean"])  # (the bands do differ)
    bank.close()


def test_refusals(capi):
    """Bad hops at sdr_create; sdr_process_device, sdr_push_kiwi_snd, sdr_graph_capture and sdr_group_create with a hop:
    each its documented status and a message in sdr_last_error."""
    import torch

    L = capi.load()

    def refused(code, fn, *args):
        rc = fn(*args)
        assert rc == code, (rc, L.sdr_last_error())
        assert len(L.sdr_last_error()) > 0

    n, rate = 4096, 192_000
    for hop in (-1, 1, 16, 100, 3000, n // 32, 2 * n, 48):
        with pytest.raises(capi.SdrError) as ei:
            capi.Bank(rate, n, hop=hop)
        assert ei.value.code == capi.ERR_BAD_ARG and len(str(ei.value)) > 0
    with pytest.raises(capi.SdrError) as ei:  # hop >= 32 although block_size / 16 is smaller
        capi.Bank(48_000, 512, hop=16)
    assert ei.value.code == capi.ERR_BAD_ARG
    for hop in (n // 16, n // 2, n):
        b = capi.Bank(rate, n, max_batch_frames=16, hop=hop)
        assert b.hop == hop
        b.close()
    bank = capi.Bank(rate, n, max_batch_frames=16, max_listeners=1, hop=n // 4)
    bank.set_stream(torch.cuda.Stream().cuda_stream)
    t = torch.zeros(16 * 2 * n + 64, dtype=torch.float32, device="cuda")
    vp = C.c_void_p
    refused(capi.ERR_STATE, L.sdr_process_device, bank._h, vp(t.data_ptr()), 4)
    refused(capi.ERR_STATE, L.sdr_process_device_sc16, bank._h, vp(t.data_ptr()), 4)
    refused(capi.ERR_STATE, L.sdr_push_kiwi_snd, bank._h, 0, rate, bytes(17 + 4 * n), 17 + 4 * n)
    refused(capi.ERR_STATE, L.sdr_graph_capture, bank._h, 4)
    refused(capi.ERR_STATE, L.sdr_graph_capture_sc16, bank._h, 4)
    # the stream call's own arguments
    span = 3 * (n // 4) + n
    refused(capi.ERR_BAD_ARG, L.sdr_process_device_stream, bank._h, vp(t.data_ptr()), 4, span - 4)  # shorter than the frames span
    refused(capi.ERR_BAD_ARG, L.sdr_process_device_stream, bank._h, vp(t.data_ptr()), 4, span + 2)  # not a multiple of 4 samples
    refused(capi.ERR_BAD_ARG, L.sdr_process_device_stream, bank._h, vp(t.data_ptr() + 8), 4, span)  # not 16-byte aligned
    refused(capi.ERR_BAD_ARG, L.sdr_process_device_stream, bank._h, vp(0), 4, span)
    refused(capi.ERR_BAD_ARG, L.sdr_process_device_stream, bank._h, vp(t.data_ptr()), 17, 16 * (n // 4) + n)  # more than max_batch_frames
    assert L.sdr_process_device_stream(bank._h, vp(t.data_ptr()), 4, span) == capi.OK
    bank.sync()
    assert bank.total_frames == 4
    bank.close()
    with pytest.raises(capi.SdrError) as ei:
        capi.Group([0], rate, n, 1, hop=n // 4)
    assert ei.value.code == capi.ERR_BAD_ARG and len(str(ei.value)) > 0
    capi.Group([0], rate, n, 1, hop=n).close()


# The carrier's level decides whether this input decodes at all, at any hop: a frame integrates 32.8 ms, so a carrier far
# above the listen threshold is "on" in every frame it touches - each mark grows by almost a frame, each gap shrinks by as
# much, and at amplitude 0.1 (90 dB over the bin's noise) the oracle reads the 3-dit gaps between letters as word gaps
# ("d l 1 a b c").  At 4.5e-5 over noise of sigma 1e-3 the carrier stands 18 dB over the noise of its 31 Hz bin (it is
# 27 dB UNDER the noise in the 2 MHz band: what the long transform is for) and a frame is "on" from about half coverage.
# Tried with the oracle alone before this test was written, 25 WPM: amplitudes 3e-5 and 6e-5 decode the call sign at
# hop = 8192 as well, 1.2e-4 and above do not; at hop = 65536 none does.
DECODE_CASE = dict(rate=2_000_000, n=65536, wpm=25, text="cq de dl1abc dl1abc dl1abc dl1abc k", repeats=1, amplitude=4.5e-5, bin=40000)


def keyed_stream(rate, n, wpm, text, repeats, amplitude, bin_, seed=31):
    """One carrier at spectrum bin `bin_` keying `text` at `wpm` over noise: float32 [samples, 2] (a whole number of
    8192-sample hops, so that the same stream serves every hop of the test)."""
    dit = int(round(1.2 / wpm * rate))  # samples
    key = np.repeat(np.concatenate([np.zeros(30, np.uint8), np.tile(synth.keying_pattern(text, 1), repeats)]), dit)
    samples = (len(key) + n + 8191) // 8192 * 8192
    key = np.concatenate([key, np.zeros(samples - len(key), np.uint8)])
    k = (bin_ + n // 2) % n
    rng = np.random.default_rng(seed)
    out = np.empty((samples, 2), np.float32)
    step = 1 << 22
    for a in range(0, samples, step):
        e = min(samples, a + step)
        ph = 2 * np.pi * ((k * np.arange(a, e, dtype=np.int64)) % n) / n
        out[a:e, 0] = amplitude * key[a:e] * np.cos(ph) + synth.NOISE_SIGMA * rng.standard_normal(e - a)
        out[a:e, 1] = amplitude * key[a:e] * np.sin(ph) + synth.NOISE_SIGMA * rng.standard_normal(e - a)
    return out


def oracle_decode(s, rate, n, hop, bin_):
    """The oracle receiver's debounced bits of one listener over every frame of s (materialised 128 frames at a time), and
    the hop-timed decoder over them."""
    r = orc.Receiver(rate, n, synth.default_edge_width(n))
    r.attach(bin_)
    r.set_find_peaks(False)
    frames = (s.shape[0] - n) // hop + 1
    deb = np.concatenate([r.process(frames_of(s, n, hop, a, min(a + 128, frames)))["deb"][:, 0] for a in range(0, frames, 128)])
    return deb, decode(deb, rate, hop)


def test_fast_keying_needs_the_hop(capi):
    """The point of the feature: 2 MS/s, N = 65536 (31 Hz bins), one carrier keying a call sign at 25 WPM (dit 48 ms) well
    above the noise.  With hop = 65536 a dit is under two ticks of 32.8 ms and the oracle's decoder does not produce the
    call sign; with hop = 8192 (tick 4.1 ms, 11.7 ticks per dit) it does.  The GPU's text equals the oracle's in both.
    The assertions on the oracle come first: a weak input fails as an input, not as a GPU mismatch."""
    import torch

    c = DECODE_CASE
    rate, n, bin_ = c["rate"], c["n"], c["bin"]
    s = keyed_stream(rate, n, c["wpm"], c["text"], c["repeats"], c["amplitude"], bin_)
    dev = torch.from_numpy(s).cuda()
    want = {}
    for hop in (n, 8192):
        deb, (text, state, _) = oracle_decode(s, rate, n, hop, bin_)
        want[hop] = (deb, text, state)
    assert "dl1abc" not in want[n][1], want[n][1]
    assert want[8192][1].count("dl1abc") >= 3, want[8192][1]
    for hop in (n, 8192):
        want_deb, text, state = want[hop]
        frames = len(want_deb)
        per = 256
        bank = capi.Bank(rate, n, max_batch_frames=per, max_listeners=1, find_peaks=False, hop=hop)
        bank.set_stream(torch.cuda.current_stream().cuda_stream)
        assert bank.attach(0, bin_) == 0
        got, deb = "", []
        for a in range(0, frames, per):
            k = min(per, frames - a)
            bank.process_device_stream(dev.data_ptr() + a * hop * 8, k, (k - 1) * hop + n)
            deb.append(bank.read_keying_bits(0, 0))
            got += bank.read_text(0, 0)
        assert np.array_equal(np.concatenate(deb), want_deb), f"hop {hop}: keying"
        assert got == text, f"hop {hop}: {got!r} != {text!r}"
        assert np.array_equal(bank.read_decoder_state(0, 0), state)
        bank.close()
