#!/usr/bin/env python3
"""What the receive chain costs over the hand-written call sequence (sdr_chain_*, csrc/capi_chain.hip), measured on the GPU
with device events, the two sides taking turns over the same device-resident input in one run, and written as JSON.

The shape is the README's fine-converter shape behind a bank: 2^24 rs16 samples per call, channelizer M = 64, D = 32, T = 512,
8 channels, fine converter D = 8, T = 128, and a bank of 8 bands (N = 512, hop 128, one listener per band, results on): 65536
narrow samples and 512 frames per band and call.  Side "hand" is INTEGRATION.md's loop written out: sdr_chan_process_device,
sdr_fine_process_device into a ring, the ring's carry moved by a strided copy when the next call would not fit, and
sdr_process_device_stream over the whole frames.  Side "chain" is one sdr_chain_push_device.  Both sides drive the SAME
channelizer, fine converter and bank, turn by turn (the chain side through a chain created for each turn, outside the timed
region, and filled by untimed pushes first), both poll the bank's results inside the timed region, and both use a ring of
the same length: once the chain's minimum, where the carry moves at every call, and once four times that.

Why one set of members: a first form of this tool gave each side objects of its own, and the side created second - the
chain's - took 0.459 ms per call against 0.348, at either ring length.  With the members shared the difference is gone
(profiles/chain_rate.json), so it belonged to the second bank in the process, not to the chain (see sdr_self_check in
the header on how HIP deals hardware queues to streams as they are created).

No ratio is fixed in advance: the yardstick is the hand-written sequence on the same box in the same run, and
"within_spread" says whether chain / hand - 1 stays within the larger of the two sides' (max - min) / median.

    python tools/chain_rate.py [--out profiles/chain_rate.json] [--rounds 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ddc_rate import N_IN, random_input  # noqa: E402
from fine_rate import L, figures  # noqa: E402

REPS = 5
BANDS, M1, D1, T1, D2, T2 = 8, 64, 32, 512, 8, 128
N, HOP, RATE = 512, 128, 48_000
NARROW = N_IN // (D1 * D2)  # per band and call


class Members:
    """Channelizer, fine converter and bank on one stream, with the tool's shape.  BOTH sides drive these same objects, turn by
    turn: two banks in one process were measured not to be equals (the module's text)."""

    def __init__(self, capi, synth, stream, channels, steps2):
        self.capi = capi
        self.bank = capi.Bank(RATE, N, n_bands=BANDS, max_batch_frames=NARROW // HOP, max_listeners=2, hop=HOP)
        self.chan = capi.Chan(M1, D1, synth.lowpass_taps(D1, T1 // D1), channels, in_format=capi.DDC_RS16, max_in_samples=N_IN)
        self.fine = capi.Fine(BANDS, D2, synth.lowpass_taps(D2, T2 // D2), steps2, max_in_samples=N_IN // D1)
        for o in (self.bank, self.chan, self.fine):
            o.set_stream(stream.cuda_stream)
        for b in range(BANDS):
            self.bank.attach(b, 100 + 37 * b)
        self.bank.enable_results(True)
        self.pending = 0

    def drain(self, wait):
        while self.pending and self.bank.poll(wait=wait, copy=False) is not None:
            self.pending -= 1

    def close(self):
        for o in (self.chan, self.fine, self.bank):
            o.close()


class Hand:
    """The hand-written sequence over a linear ring of `ring` samples per band, the chain's arithmetic written out.  Its
    sample and frame counts are its own (the bank's frames are not one continuous stream in this tool: the sides take turns)."""

    def __init__(self, members, ring):
        import torch

        self.m = members
        self.n1 = N_IN // D1
        self.mid = torch.empty((BANDS, self.n1, 2), dtype=torch.float32, device="cuda")
        self.ring = torch.zeros((BANDS, ring, 2), dtype=torch.float32, device="cuda")
        self.size, self.base, self.have, self.done, self.moves, self.calls = ring, 0, 0, 0, 0, 0

    def call(self, x):
        m = self.m
        if self.have - self.base + NARROW > self.size:
            nxt = self.done * HOP
            keep = self.have - nxt
            if keep:
                self.ring[:, :keep] = self.ring[:, nxt - self.base:self.have - self.base]  # (source and destination do not overlap)
            self.base = nxt
            self.moves += 1
        m.chan.process_device(x.data_ptr(), N_IN, self.mid.data_ptr(), self.n1)
        m.fine.process_device(self.mid.data_ptr(), self.n1, self.n1, self.ring.data_ptr() + (self.have - self.base) * 8, self.size)
        self.have += NARROW
        k = (self.have - self.done * HOP - N) // HOP + 1
        m.bank.process_device_stream(self.ring.data_ptr() + (self.done * HOP - self.base) * 8, k, self.size)
        self.done += k
        self.calls += 1
        m.pending += 1
        m.drain(False)


class Chained:
    """One sdr_chain_push_device per call.  A chain notices members driven by hand between its pushes, so every turn gets a
    chain of its own over the shared members (created and destroyed outside the timed region) and begins with start()
    untimed pushes, after which the ring is as full as in the steady state."""

    def __init__(self, members, ring):
        self.m, self.size, self.chain, self.moves, self.calls = members, ring, None, 0, 0

    def start(self, x, pushes):
        self.chain = self.m.capi.Chain(self.m.bank, chan=self.m.chan, fine=self.m.fine, max_in_samples=N_IN, ring_samples=self.size)
        for _ in range(pushes):
            self.call(x)
        self.m.drain(True)
        self.calls -= pushes
        self.before = self.chain.stats()["carry_moves"]

    def call(self, x):
        self.m.pending += self.chain.push_device(x.data_ptr(), N_IN)
        self.calls += 1
        self.m.drain(False)

    def stop(self):
        self.moves += self.chain.stats()["carry_moves"] - self.before
        self.chain.close()
        self.chain = None


def timed(stream, members, side, x, reps):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        side.call(x)
    members.drain(True)
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def pair(members, stream, x, ring, rounds):
    hand, chain = Hand(members, ring), Chained(members, ring)
    fill = -(-ring // NARROW)  # pushes until the ring has been full once
    timed(stream, members, hand, x, 4 + fill)
    hand.moves = hand.calls = 0
    chain.start(x, 4 + fill)
    chain.stop()
    chain.moves = 0
    runs = {"hand": [], "chain": []}
    for _ in range(rounds):
        runs["hand"].append(timed(stream, members, hand, x, REPS))
        chain.start(x, fill)
        runs["chain"].append(timed(stream, members, chain, x, REPS))
        chain.stop()
    res = {"ring_samples": ring, "hand": figures(runs["hand"]), "chain": figures(runs["chain"]),
           "timed_calls": {"hand": hand.calls, "chain": chain.calls}, "carry_moves_in_timed_calls": {"hand": hand.moves, "chain": chain.moves}}
    res["chain_over_hand_time"] = res["chain"]["ms_per_call"] / res["hand"]["ms_per_call"]
    res["allowed_excess"] = max(res["hand"]["spread"], res["chain"]["spread"])
    res["within_spread"] = bool(res["chain_over_hand_time"] - 1.0 <= res["allowed_excess"])
    for name in ("hand", "chain"):
        res[name]["input_gsps"] = N_IN / (res[name]["ms_per_call"] * 1e-3) / 1e9
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_rate.json"))
    ap.add_argument("--rounds", type=int, default=20, help="rounds of 5 calls per side (20 for a figure that is quoted)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("chain_rate.py measures on the GPU: none is available (there is nothing to report without one)")
    from sdrainer_amd.csrc import build
    build.build()
    from sdrainer_amd import capi, synth

    targets = [int((b - 3.6) * L * D1 / 8) + 3000 * (b + 1) for b in range(BANDS)]  # tools/fine_rate.py's: off the channel grid
    tuned = [capi.fine_tune(M1, D1, t) for t in targets]
    channels, steps2 = [c for c, _ in tuned], [s for _, s in tuned]
    minimum = capi.chain_min_ring(N, HOP, N_IN, D1 * D2)
    stream = torch.cuda.Stream()
    res = {"device": torch.cuda.get_device_name(0), "input": "rs16", "input_samples_per_call": N_IN, "bands": BANDS,
           "channelizer": dict(channels_of=M1, decimation=D1, taps=T1, channels=channels), "fine": dict(decimation=D2, taps=T2, steps=steps2),
           "bank": dict(block_size=N, hop=HOP, frames_per_call=NARROW // HOP, listeners_per_band=1), "rounds": args.rounds, "calls_per_timing": REPS,
           "timing": "device events around 5 back-to-back calls on one stream with the finished batches polled after every call and the rest "
                     "waited for inside the timed region, behind a warm-up; the sides take turns; medians over the rounds",
           "not_measured": "sdr_chain_push_host, other input formats and shapes, a blanker in the chain, a second box (the box-to-box spread)"}
    with torch.cuda.stream(stream):
        x = random_input(capi, "rs16", 5)
        members = Members(capi, synth, stream, channels, steps2)
        for name, ring in (("minimum_ring", minimum), ("four_times_the_minimum", 4 * minimum)):
            r = res[name] = pair(members, stream, x, ring, args.rounds)
            print(f"ring {ring}: hand {r['hand']['ms_per_call']:.3f} ms/call, chain {r['chain']['ms_per_call']:.3f} ms/call: "
                  f"{r['chain_over_hand_time']:.3f}x (allowed excess {r['allowed_excess']:.3f}, within: {r['within_spread']}); "
                  f"carry moves {r['carry_moves_in_timed_calls']['chain']} in {r['timed_calls']['chain']} timed calls "
                  f"(hand: {r['carry_moves_in_timed_calls']['hand']} in {r['timed_calls']['hand']})", flush=True)
        members.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
