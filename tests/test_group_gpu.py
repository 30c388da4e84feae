"""sdr_group on the GPU: a group of two members on device 0 (and on devices 0 and 1 where two GPUs are visible) driven
side by side with ONE bank of the same five bands.  Every merged delivery equals the bank's, field by field; one band's
frame records, psd and text equal the oracle's; staged input, a collective setter between batches, deferred listening,
a too-small buffer, a consumer thread and the caller's current device behave as the header says."""
import ctypes as C
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import oracle as orc  # noqa: E402
from parity_tools import (GROUP_BANDS as BANDS, GROUP_CENTER as CENTER, Pair, assert_records_equal, capi, group_bands as _bands,  # noqa: E402, F401
                          same_delivery as _same)
from sdrainer_amd import synth  # noqa: E402

DEVICE_SETS = [pytest.param((0, 0), id="dev00"),
               pytest.param((0, 1), id="dev01", marks=pytest.mark.skipif(
                   not torch.cuda.is_available() or torch.cuda.device_count() < 2, reason="needs two visible GPUs"))]


def _text(res, band, texts):
    for r in res["listeners"]:
        if int(r["band"]) == band:
            lid = int(r["listener"])
            texts[lid] = texts.get(lid, "") + "".join(chr(int(x)) for x in res["runes"][r["first_rune"]:r["first_rune"] + r["n_runes"]])


@pytest.mark.parametrize("devices", DEVICE_SETS)
@pytest.mark.parametrize("n,rate,batches", [(1024, 96000, (100, 250, 350)), (16384, 768000, (100, 60, 140))], ids=["n1024", "n16384"])
def test_group_delivers_what_one_bank_delivers(capi, devices, n, rate, batches):
    tones, frames, band = 4, sum(batches), 3  # band 3: member 1, local band 1
    edge = synth.default_edge_width(n)
    iq, bins = _bands(frames, rate, n, tones, seed=5100 + n)
    p = Pair(capi, devices, rate, n, edge_width=edge, max_listeners=8, max_batch_frames=max(batches), max_peaks=64)
    p.bank.enable_results(True)
    p.group.enable_results(True)
    p.check_device()
    ref = orc.Receiver(rate, n, edge, 15.0, 1, center_frequency=CENTER[band])
    texts, f0, delivered = {}, 0, 0
    for k, nf in enumerate(batches):
        seg = iq[:, f0:f0 + nf]
        p.process(seg)
        last = k == len(batches) - 1
        want = ref.process(seg[band], want_spectrum=last)
        res = p.polls()
        assert res["batch_index"] == k and res["first_frame"] == f0 and res["n_frames"] == nf
        delivered += 1
        _text(res, band, texts)
        m, lb = p.group.member(band)
        assert_records_equal(m.read_frame_records(lb), want["frames"])
        if last:
            _, psd = m.read_spectrum(lb, nf - 1)
            assert np.array_equal(psd.view(np.uint32), want["psd"][-1].view(np.uint32))
        if k == 0:  # listeners behind the first cumulation, on every band
            for b in range(BANDS):
                for t in bins[b]:
                    p.attach(b, t)
            for t in bins[band]:
                ref.attach(int(t))
        f0 += nf
    assert p.polls(wait=False) is None
    for lid in range(tones):
        assert texts.get(lid, "") == ref.text(lid), lid
    assert sum(len(t) for t in texts.values()) > 0 or n == 16384  # (few frames at N=16384: maybe no whole rune yet)
    assert p.group.read_drop_counters() == p.bank.read_drop_counters() == (0, 0)
    p.check_device()
    p.close()


def test_staged_input_takes_the_minimum_over_every_band(capi):
    n, rate, tones = 1024, 96000, 3
    iq, bins = _bands(600, rate, n, tones, seed=5300)
    p = Pair(capi, (0, 0), rate, n, max_listeners=4, max_batch_frames=512, max_peaks=64)
    p.bank.enable_results(True)
    p.group.enable_results(True)
    for b in range(BANDS):
        p.attach(b, bins[b][0])
    pushed = [0] * BANDS

    def push(counts):
        for b, c in enumerate(counts):
            if c:
                seg = iq[b, pushed[b]:pushed[b] + c]
                assert p.bank.push_iq(b, rate, seg) == capi.OK
                assert p.group.push_iq(b, rate, seg) == capi.OK
                pushed[b] += c
        p.check_device()

    push([300, 180, 250, 0, 400])  # band 3 (member 1) has nothing: the whole group waits, as one bank does
    assert p.bank.process_staged() == 0 and p.group.process_staged() == 0
    push([0, 0, 0, 120, 0])
    assert p.bank.process_staged() == 120 and p.group.process_staged() == 120
    p.check_device()
    for b in range(BANDS):
        m, lb = p.group.member(b)
        assert m.staged_frames(lb) == p.bank.staged_frames(b) == pushed[b] - 120
    p.polls()
    push([0, 100, 0, 200, 0])
    assert p.bank.process_staged_limit(100) == 100 and p.group.process_staged_limit(100) == 100
    p.polls()
    assert p.bank.process_staged() == 30 and p.group.process_staged() == 30  # band 2: 250 pushed, 220 consumed
    p.polls()
    assert p.polls(wait=False) is None
    # the wrong sample rate is the bank's log-and-drop case, routed
    assert p.group.push_iq(2, rate + 1, iq[2, :1]) == capi.ERR_BAD_RATE
    p.close()


def test_collective_setter_between_batches(capi):
    n, rate, tones, per = 1024, 96000, 3, 150
    edge = synth.default_edge_width(n)
    iq, bins = _bands(3 * per, rate, n, tones, seed=5400)
    group = capi.Group((0, 0), rate, n, BANDS, edge_width=edge, max_listeners=4, max_batch_frames=per)
    refs = []
    for b in range(BANDS):
        m, lb = group.member(b)
        refs.append(orc.Receiver(rate, n, edge, 15.0, 1))
        for t in bins[b]:
            m.attach(lb, int(t))
            refs[b].attach(int(t))
    # batch 0 at the default, batch 1 everywhere at 9, batch 2 everywhere at 21.5 but band 4 at 30
    plan = [(None, {}), (9.0, {}), (21.5, {4: 30.0})]
    for k, (everywhere, per_band) in enumerate(plan):
        if everywhere is not None:
            group.set_peak_threshold(-1, everywhere)
        for b, t in per_band.items():
            group.set_peak_threshold(b, t)
        ts = [torch.from_numpy(np.ascontiguousarray(iq[m::2, k * per:(k + 1) * per])).to("cuda:0") for m in range(2)]
        group.process_device([t.data_ptr() for t in ts], per)
        group.sync()
        for b in range(BANDS):
            t = per_band.get(b, everywhere)
            if t is not None:
                refs[b].set_peak_threshold(t)
            want = refs[b].process(iq[b, k * per:(k + 1) * per])
            m, lb = group.member(b)
            got = m.read_frame_records(lb)
            assert got["peak_thr"].view(np.uint32).tolist() == want["frames"]["peak_thr"].view(np.uint32).tolist(), (k, b)
    with pytest.raises(capi.SdrError):
        group.set_peak_threshold(BANDS, 1.0)
    group.close()


def test_deferred_listen_over_the_group(capi):
    n, rate, tones = 1024, 96000, 4
    edge = synth.default_edge_width(n)
    iq, bins = _bands(730, rate, n, tones, seed=5500)
    p = Pair(capi, (0, 0), rate, n, edge_width=edge, max_listeners=8, max_batch_frames=512, max_peaks=64)
    p.bank.enable_results(True)
    p.group.enable_results(True)
    p.bank.defer_listen(True)
    p.group.defer_listen(True)
    bound = 0
    for a, e in ((0, 450), (450, 730)):
        p.process(iq[:, a:e])
        pk_bank, pk_group = p.bank.poll_peaks(wait=True), p.group.poll_peaks(wait=True)
        p.check_device()
        _same(pk_group, pk_bank)
        assert len(pk_group["listeners"]) == 0 and len(pk_group["chunks"]) > 0
        nxt = p.member_input(iq[:, e - 10:e])
        with pytest.raises(capi.SdrError) as err:  # the members wait for their listen half
            p.group.process_device([x.data_ptr() for x in nxt], 10)
        assert err.value.code == capi.ERR_STATE
        # one listener per completed cumulation, on the strongest peak of that chunk, hearing the next frame
        for c in pk_bank["chunks"]:
            if c["n_peaks"] == 0:
                continue
            pk = pk_bank["peaks"][c["first_peak"]:c["first_peak"] + c["n_peaks"]]
            best = pk[int(np.argmax(pk["signal_value"]))]
            band, start = int(c["band"]), int(c["frame"]) + 1
            lid = p.bank.attach_at(band, int(best["signal_bin"]), start)
            m, lb = p.group.member(band)
            assert m.attach_at(lb, int(best["signal_bin"]), start) == lid
            bound += 1
        p.bank.process_listen()
        p.group.process_listen()
        p.check_device()
        res = p.polls()
        assert res["first_frame"] == a and res["n_frames"] == e - a
    assert bound > 0
    with pytest.raises(capi.SdrError):
        p.group.process_listen()  # nothing waits
    p.bank.defer_listen(False)
    p.group.defer_listen(False)
    p.close()


def test_poll_bad_size_then_retry_and_a_consumer_thread(capi):
    n, rate, tones, per, batches = 1024, 96000, 4, 100, 8
    iq, bins = _bands(per * (batches + 1), rate, n, tones, seed=5600)
    p = Pair(capi, (0, 0), rate, n, max_listeners=8, max_batch_frames=per, max_peaks=64)
    p.bank.enable_results(True)
    p.group.enable_results(True)
    p.process(iq[:, :per])
    for b in range(BANDS):
        for t in bins[b]:
            p.attach(b, t)
    p.process(iq[:, per:2 * per])
    # BAD_SIZE: the n_* fields say what is needed, nothing is delivered, the members' batches stay with the group
    small = capi.Results()
    small.struct_size = C.sizeof(capi.Results)
    L = capi.load()
    assert L.sdr_group_poll(p.group._h, C.byref(small), 1) == capi.ERR_BAD_SIZE
    assert small.batch_index == 0 and small.n_chunks == BANDS
    assert p.bank.results_pending == 2
    first = p.bank.poll(wait=True)
    again = p.group.poll(wait=True)
    _same(again, first)
    assert small.n_peaks == len(again["peaks"]) and small.n_listeners == len(again["listeners"])
    second = p.bank.poll(wait=True)
    _same(p.group.poll(wait=True), second)
    assert len(second["listeners"]) > 0
    # a consumer thread polls while the producer processes: every batch once, in order, equal to the bank's
    got, err = [], []

    def consume():
        try:
            while len(got) < batches - 1:
                r = p.group.poll(wait=True)
                if r is not None:
                    got.append(r)
        except Exception as ex:  # (reported by the main thread)
            err.append(ex)

    th = threading.Thread(target=consume)
    th.start()
    want = []
    for k in range(2, batches + 1):
        seg = iq[:, k * per:(k + 1) * per]
        ts = p.member_input(seg)
        p.group.process_device([x.data_ptr() for x in ts], per)
        t = torch.from_numpy(np.ascontiguousarray(seg)).to("cuda:0")
        p.bank.process_device(t.data_ptr(), per)
        p.bank.sync()
        want.append(p.bank.poll(wait=True))
    th.join(timeout=300)
    assert not th.is_alive() and not err, err
    assert [r["batch_index"] for r in got] == list(range(2, batches + 1))
    for a, b in zip(got, want):
        _same(a, b)
    p.check_device()
    p.close()


def test_group_checks_before_it_launches(capi):
    n, rate = 1024, 96000
    with pytest.raises(capi.SdrError) as e:
        capi.Group((0, 0), rate, n, 1)  # fewer bands than members
    assert e.value.code == capi.ERR_BAD_ARG
    g = capi.Group((0, 0), rate, n, 3, max_batch_frames=100, max_listeners=2)
    iq = 1e-3 * torch.randn((2, 100, 2 * n), dtype=torch.float32, device="cuda:0")
    with pytest.raises(capi.SdrError) as e:
        g.process_device([iq[0].data_ptr(), iq[1].data_ptr() + 4], 100)  # misaligned: refused before any member runs
    assert e.value.code == capi.ERR_BAD_ARG
    with pytest.raises(capi.SdrError) as e:
        g.process_device([iq[0].data_ptr(), iq[1].data_ptr()], 101)
    assert e.value.code == capi.ERR_BAD_ARG
    # graph mode is out of scope: a member captured through sdr_group_member stops the group's processing calls
    stream = torch.cuda.Stream(device=0)
    m, _ = g.member(0)
    m.set_stream(stream.cuda_stream)
    m.graph_capture(50)
    with pytest.raises(capi.SdrError) as e:
        g.process_device([iq[0].data_ptr(), iq[1].data_ptr()], 50)
    assert e.value.code == capi.ERR_STATE
    m.graph_release()
    g.process_device([iq[0].data_ptr(), iq[1].data_ptr()], 50)  # nothing ran out of step: the group works on
    g.sync()
    assert g.member(0)[0].total_frames == g.member(1)[0].total_frames == 50
    g.close()
