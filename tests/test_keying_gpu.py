"""k_listen_decode itself - not its stage functions on the host (tests/emu/emu_stages.cpp) - under hostile keying, against
the CPU oracle, bit for bit: speeds that change inside the stream, jitter, glitches, over-long marks, long silences,
characters of more than eight symbols, runs of dahs, plain noise, and listeners with hundreds of edges per batch beside idle
ones in one workgroup.  The inputs and what they are for are tests/keying_gen.py's; tests/test_keying_reach.py asserts, on
the CPU, that they reach the kernel's paths: rounds whose LDS rings wrap, an abort pending across a round and a batch, the
character taken in front of a batch's first edge, a ninth symbol, more than eight das in a round, a workgroup across two
bands, a half-wave without its partner, stage 0's second chunk of 64 words, sdr_attach_at in the middle of a character.

Cases (a) - (d) go through parity_case.Case with trace: keying bits raw and debounced, edges, runes and their frames,
decoder state and drop counters of 0, every listener, every batch.  (e) and (f) drive the bank themselves.  Every comparison
is exact."""
import numpy as np
import pytest

import keying_gen as gen
from oracle import oracle as orc
from parity_tools import capi  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu


def test_base(capi):
    """(a): 38 slots of two bands in three workgroups, every kind in each; batches of 1, 63, 64, 65 and 1024 frames and two
    cut by the oracle's edges (64 and 33 edges of one listener); a listener attached late beside its half-wave partner."""
    case = gen.case_a()
    bank = case.run(capi)
    bank.close()


@pytest.mark.parametrize("row", range(len(gen.B_ROWS)), ids=[f"debounce{d}x{len(s)}" for d, s in gen.B_ROWS])
def test_debounce(capi, row):
    """(b): noise and jitter through debounces of 2, 3, 5, 9 and 70; one batch of 4200 frames, whose last words are stage 0's
    second chunk."""
    case = gen.case_b(row)
    bank = case.run(capi, activity=False)  # (a debounce of 70 lets an edge or two per listener through: the floor is below)
    assert case.edges >= 12, case.edges
    bank.close()


def test_deferred(capi):
    """(c): sdr_attach_at at frames 64, 130 and the last one of a deferred batch of 1024, onto carriers in mid-character."""
    case = gen.case_c()
    bank = case.run(capi)
    late = len(gen.C_KINDS) - len(gen.C_LATE)
    assert all(len(case.text[0][lid]) > 0 for lid in (late, late + 1)), "the listeners bound inside the batch wrote nothing"
    bank.close()


def test_graph(capi):
    """(d): the same kinds through hipGraph replays."""
    case = gen.case_d_graph()
    bank = case.run(capi)
    bank.close()


def test_overlapped(capi):
    """(d): a hop of N / 4 at N = 2048 on the device stream path: the decoder's tick is the hop, every speed term another."""
    case = gen.case_d_hop()
    bank = case.run(capi)
    bank.close()


@pytest.mark.parametrize("which", [0, 1], ids=["pending", "pending_invalid"])
def test_stop_inside_a_character(capi, which):
    """(e): the stream is cut two frames behind a mark, with a character pending (an ordinary one; an invalid one, its last
    mark the over-long one); sdr_listener_stop writes it as Decoder.stop() does, for every listener of the band."""
    band, cuts = gen.e_input()
    f32, _, bins = band
    cut = cuts[which]
    deb = gen.oracle_bits(gen.N, gen.RATE, f32, bins)
    bank = capi.Bank(gen.RATE, gen.N, max_batch_frames=1024, max_listeners=len(bins), trace=True, find_peaks=False)
    for lid, b in enumerate(bins):
        assert bank.attach(0, b) == lid
    for a, e in ((0, 300), (300, cut)):
        bank.process_host(f32[a:e])
        for lid in range(len(bins)):
            assert np.array_equal(bank.read_trace(0, lid)[2], deb[a:e, lid]), (lid, a)
    added = []
    for lid in range(len(bins)):
        d = orc.Decoder(gen.RATE, gen.N)
        d.reset()
        d.ticks(deb[:cut, lid])
        before = d.text()
        d.stop()
        added.append(d.text()[len(before):])
        bank.listener_stop(0, lid)
        assert bank.read_text(0, lid) == d.text(), f"listener {lid}"
    assert added[0] == ("a", "\xa6")[which], added
    assert bank.read_drop_counters() == (0, 0)
    bank.close()


def test_text_capacity_held_to_the_oracle(capi):
    """(f): nothing is read while three fast listeners and a clean one of one workgroup write, until by the oracle every fast
    one has passed the 2048 runes its buffer holds by 100 and more.  Each text is the oracle's first 2048 runes (all of the
    clean one's), the runes counted as dropped are exactly the overflow, no edge is dropped."""
    import torch

    band, batches, decs = gen.f_input()
    f32, _, bins = band
    bank = capi.Bank(gen.RATE, gen.N, max_batch_frames=gen.F_BATCH, max_listeners=len(bins), find_peaks=False)
    bank.set_stream(torch.cuda.current_stream().cuda_stream)
    for lid, b in enumerate(bins):
        assert bank.attach(0, b) == lid
    dev = torch.from_numpy(f32).cuda()
    for k in range(batches):
        bank.process_device(dev[k * gen.F_BATCH:(k + 1) * gen.F_BATCH].data_ptr(), gen.F_BATCH)
    bank.sync()
    assert bank.total_frames == batches * gen.F_BATCH
    overflow = sum(max(0, len(text) - gen.TEXT_CAP) for text, _ in decs)
    assert overflow >= 3 * gen.F_OVER
    assert bank.read_drop_counters() == (overflow, 0)
    for lid, (text, _) in enumerate(decs):
        got = bank.read_text(0, lid)
        assert len(got) == min(len(text), gen.TEXT_CAP), f"listener {lid}: {len(got)} runes kept of {len(text)}"
        assert got == text[:gen.TEXT_CAP], f"listener {lid}"
    bank.close()
