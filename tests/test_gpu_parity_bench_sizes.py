"""GPU parity at the sizes bench.py runs ("do this" 1): the HIP path through its C ABI against the CPU
oracle, bit for bit, on the benchmark's own generator (synth.make_band_torch) and batch geometry.

  config 3   N = 16384, 256 listeners, 2048-frame batches (two of them: everything carried between batches) and the
             bench's default 8192-frame batch
  config 2   N = 4096, 16 listeners, 4096-frame batches
  config 5   8 channels x N = 8192 x 16 listeners, 2048-frame batches (the per-GPU share), eager and as hipGraph replays

What is compared per batch: frame records (min mean, variance, dB inputs, rolling means, thresholds), every listener's
debounced keying bits, keying edges, decoded text and decoder state (12 float64), every completed cumulation and its
peak list (bins, values, float64 -> int frequencies).  The oracle needs 30 MS/s per core; bands run on threads of their
own (ctypes releases the GIL).
"""
import numpy as np
import pytest

from oracle import oracle as orc
from parity_case import Case
from parity_tools import REC_FIELDS, bits_equal, capi, check_batch_polled, run_oracle  # noqa: F401 (capi: the fixture)
from sdrainer_amd import synth

pytestmark = pytest.mark.gpu


def test_config3_at_bench_size(capi):
    """bench.py's default workload: N = 16384, 256 listeners, two 2048-frame batches (decoder 4 signals per wave,
    80-workgroup window sums, 21-cumulation batches: the geometry the throughput number is quoted on)."""
    Case(16384, 1, 256, 256, [("batch", 2048)] * 2, seed=3000).run(capi).close()


def test_config3_at_bench_default_batch(capi):
    """bench.py's default batch for config 3: 8192 frames (82 cumulations per batch, 128-word keying rows, four times
    the edges and runes per delivery), then a short batch behind it for everything that is carried over."""
    Case(16384, 1, 256, 256, [("batch", 8192), ("batch", 300)], seed=3100).run(capi).close()


def test_config2_at_bench_size(capi):
    """bench.py --workload c2: N = 4096, 16 listeners (a decoder wave each), 4096-frame batches."""
    Case(4096, 1, 16, 16, [("batch", 4096)] * 2, seed=2000, rate=192_000, free_last=False).run(capi).close()


def test_config5_share_at_bench_size(capi):
    """bench.py --workload c5: 8 channels x 8192 points x 16 listeners per GPU, 2048-frame batches."""
    Case(8192, 8, 16, 16, [("batch", 2048)] * 2, seed=5000, free_last=False).run(capi).close()


def test_graph_mode_at_config5_geometry(capi):
    """hipGraph replays at config 5's geometry (8 bands x 8192 x 16 listeners; device-side cursors for 8 bands): two
    replays of sdr_graph_batches() batches of 460 frames - cumulation phase, carry buffer and frame numbering differ
    from batch to batch - against the oracle: delivery (edges, runes, peaks), records, bits, decoder state."""
    import torch

    rate, n, tones, n_bands, per = 2_000_000, 8192, 16, 8, 460
    edge = synth.default_edge_width(n)
    bank = capi.Bank(rate, n, n_bands=n_bands, edge_width=edge, max_batch_frames=per, max_listeners=tones, max_peaks=256)
    K = bank.graph_batches
    total = 2 * K * per
    dev_iq, bins_per_band, host_iq = [], [], []
    for b in range(n_bands):
        iq, bins, _ = synth.make_band_torch(total, rate, n, tones, seed=5500 + 17 * b, device="cuda")
        dev_iq.append(iq)
        bins_per_band.append(bins)
        host_iq.append(iq.cpu().numpy())
    centers = [7000000 + 50000 * b for b in range(n_bands)]
    refs, outs, _ = run_oracle(rate, n, edge, bins_per_band, host_iq, centers)
    stream = torch.cuda.Stream()
    bank.set_stream(stream.cuda_stream)
    for b in range(n_bands):
        bank.set_center_frequency(b, centers[b])
        for i, bn in enumerate(bins_per_band[b]):
            assert bank.attach(b, int(bn)) == i
    bank.enable_results(True)
    bank.graph_capture(per)
    batches = [torch.stack([iq[k * per:(k + 1) * per] for iq in dev_iq]).contiguous() for k in range(2 * K)]
    torch.cuda.synchronize()
    text = [["" for _ in range(tones)] for _ in range(n_bands)]
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
    assert bank.total_frames == total
    for b in range(n_bands):
        recs = bank.read_frame_records(b)
        for f in REC_FIELDS:
            assert bits_equal(recs[f], outs[b]["frames"][f][total - per:].copy()), f"band {b} field {f}"
        for lid in range(tones):
            assert text[b][lid] == refs[b].text(lid), f"band {b} listener {lid}"
            assert np.array_equal(bank.read_keying_bits(b, lid), outs[b]["deb"][total - per:, lid])
            assert np.array_equal(bank.read_decoder_state(b, lid), refs[b].decoder_state(lid))
    # attaching or detaching invalidates the capture (include/sdrainer_hip.h)
    bank.detach(0, 3)
    with pytest.raises(capi.SdrError) as ei:
        bank.graph_launch([batches[0].data_ptr()] * K)
    assert ei.value.code == capi.ERR_STATE
    bank.close()


def test_listeners_bound_inside_a_batch_at_config3_size(capi):
    """The deferred listen half at config 3's geometry (N = 16384, a 2048-frame batch): twenty listeners bound one per
    cumulation boundary INSIDE the batch (sdr_attach_at: gather from the retained psd rows, decoders starting mid-batch)
    beside 64 that were there from the start, against the oracle run cumulation by cumulation with a plain attach at
    every boundary (rx/receiver.go:404-426)."""
    import torch

    rate, n, frames = 2_000_000, 16384, 2048
    early, late = 64, 20
    edge = synth.default_edge_width(n)
    iq, bins, _ = synth.make_band_torch(frames, rate, n, early + late, seed=3300, device="cuda", free_last_window=True)
    host = iq.cpu().numpy()
    ref = orc.Receiver(rate, n, edge, 15.0, 1, center_frequency=14000000)
    for b in bins[:early]:
        ref.attach(int(b))
    starts = {}
    outs, pos = [], 0
    for j in range(late):
        boundary = 100 * (j + 1)
        outs.append((pos, ref.process(host[pos:boundary])))
        pos = boundary
        starts[ref.attach(int(bins[early + j]))] = boundary
    outs.append((pos, ref.process(host[pos:])))

    bank = capi.Bank(rate, n, edge_width=edge, max_batch_frames=frames, max_listeners=early + late, max_peaks=1024)
    bank.set_stream(torch.cuda.current_stream().cuda_stream)
    bank.set_center_frequency(0, 14000000)
    for i, b in enumerate(bins[:early]):
        assert bank.attach(0, int(b)) == i
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
        for base, out in outs:
            if out["deb"].shape[1] <= lid or base + out["deb"].shape[0] <= s:
                continue
            deb = out["deb"][:, lid].astype(np.int8)
            idx = np.flatnonzero(np.diff(np.concatenate([[last], deb])) != 0)
            want += [(base + int(i), int(deb[i])) for i in idx if base + i >= s]
            last = int(deb[-1])
        r = by.get(lid)
        got = [] if r is None else [(int(x["frame"]), int(x["state"])) for x in res["edges"][r["first_edge"]:r["first_edge"] + r["n_edges"]]]
        assert got == want, f"listener {lid} (from frame {s})"
        text = "" if r is None else "".join(chr(int(x)) for x in res["runes"][r["first_rune"]:r["first_rune"] + r["n_runes"]])
        assert text == ref.text(lid), f"listener {lid} text"
        assert np.array_equal(bank.read_decoder_state(0, lid), ref.decoder_state(lid)), f"listener {lid} state"
        n_edges += len(got)
    assert n_edges > 20 * early
    bank.close()
