#!/usr/bin/env python3
"""What the fine converter costs (sdr_fine_*, csrc/k_fine.hip), measured on the GPU with device events, the sides taking
turns over the same device-resident input in one run, and written as JSON.

1. Against the only way there was: 8 bands from 8 float32 streams of 2^19 samples per call, D = 8, T = 128 - one sdr_fine
   call (2 launches) against eight one-band SDR_DDC_F32 sdr_ddc objects on the same HIP stream (16 launches), the same
   arithmetic.  The fine call's median must not exceed the eight objects' median by more than the larger of the two sides'
   (max - min) / median over the rounds; "within_spread" says whether it does.
2. The point of the feature: 2^24 rs16 samples per call, 8 bands at centres off the channel grid, total decimation 256 -
   sdr_ddc at D = 256, T = 2048 against sdr_chan (M = 64, D = 32, T = 512, the 8 channels sdr_fine_tune names) followed by
   sdr_fine (D = 8, T = 128); ms per call for both sides and for the fine stage alone, and the ratio.

20 rounds of 10 calls per side behind a warm-up; medians.

    python tools/fine_rate.py [--out profiles/fine_rate.json] [--rounds 20]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ddc_rate import N_IN, random_input, timed  # noqa: E402

REPS = 10
L = 65536


def take_turns(stream, side, rounds):
    """{name: seconds per call, one figure per round}: a warm-up of every side, then the sides alternate."""
    for fn in side.values():
        timed(stream, fn, 20)
    runs = {name: [] for name in side}
    for _ in range(rounds):
        for name, fn in side.items():
            runs[name].append(timed(stream, fn, REPS))
    return runs


def figures(runs):
    med = float(np.median(runs))
    return {"ms_per_call": med * 1e3, "min_ms": min(runs) * 1e3, "max_ms": max(runs) * 1e3, "spread": (max(runs) - min(runs)) / med,
            "runs_ms": [r * 1e3 for r in runs]}


def against_eight_ddcs(capi, synth, stream, rounds):
    import torch

    bands, n, d, t = 8, 1 << 19, 8, 128
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    x = torch.rand((bands, n, 2), dtype=torch.float32, device="cuda", generator=g) * 2 - 1
    m = n // d
    out = torch.empty((bands, m, 2), dtype=torch.float32, device="cuda")
    taps = synth.lowpass_taps(d, t // d)
    steps = [-28000 + 8000 * b for b in range(bands)]
    fine = capi.Fine(bands, d, taps, steps, max_in_samples=n)
    fine.set_stream(stream.cuda_stream)
    ddcs = [capi.Ddc(d, taps, [s], in_format=capi.DDC_F32, max_in_samples=n) for s in steps]
    for ddc in ddcs:
        ddc.set_stream(stream.cuda_stream)

    def eight():
        for b, ddc in enumerate(ddcs):
            ddc.process_device(x.data_ptr() + b * n * 8, n, out.data_ptr() + b * m * 8, m)

    runs = take_turns(stream, {"fine": lambda: fine.process_device(x.data_ptr(), n, n, out.data_ptr(), m), "eight_ddcs": eight}, rounds)
    fine.close()
    for ddc in ddcs:
        ddc.close()
    res = {"bands": bands, "inputs": bands, "decimation": d, "taps": t, "samples_per_input_and_call": n, "rounds": rounds,
           "calls_per_timing": REPS, "launches_per_call": {"fine": 2, "eight_ddcs": 16},
           "fine": figures(runs["fine"]), "eight_ddcs": figures(runs["eight_ddcs"])}
    res["fine_over_eight_ddcs_time"] = res["fine"]["ms_per_call"] / res["eight_ddcs"]["ms_per_call"]
    res["allowed_excess"] = max(res["fine"]["spread"], res["eight_ddcs"]["spread"])
    res["within_spread"] = bool(res["fine_over_eight_ddcs_time"] - 1.0 <= res["allowed_excess"])
    return res


def chain_against_ddc(capi, synth, stream, rounds):
    import torch

    bands, m1, d1, t1, d2, t2, dd, td = 8, 64, 32, 512, 8, 128, 256, 2048
    # centres off the channel grid, in units of wide_rate / (65536 * d1): one band per 1/8 of the wide stream, each a good way
    # from its channel's centre
    targets = [int((b - 3.6) * L * d1 / 8) + 3000 * (b + 1) for b in range(bands)]
    tuned = [capi.fine_tune(m1, d1, target) for target in targets]
    channels, steps2 = [c for c, _ in tuned], [s for _, s in tuned]
    assert len(set(channels)) == bands and all(s != 0 for s in steps2)
    # the one-DDC side's steps: the same centres in units of wide_rate / 65536 (rounded: the cost does not depend on them)
    steps = [max(-32768, min(32767, round(target / d1))) for target in targets]
    x = random_input(capi, "rs16", 5)
    n1 = N_IN // d1
    n2 = n1 // d2
    mid = torch.empty((bands, n1, 2), dtype=torch.float32, device="cuda")
    out = torch.empty((bands, n2, 2), dtype=torch.float32, device="cuda")
    ddc = capi.Ddc(dd, synth.lowpass_taps(dd, td // dd), steps, in_format=capi.DDC_RS16, max_in_samples=N_IN)
    chan = capi.Chan(m1, d1, synth.lowpass_taps(d1, t1 // d1), channels, in_format=capi.DDC_RS16, max_in_samples=N_IN)
    fine = capi.Fine(bands, d2, synth.lowpass_taps(d2, t2 // d2), steps2, max_in_samples=n1)
    for obj in (ddc, chan, fine):
        obj.set_stream(stream.cuda_stream)
    assert N_IN // dd == n2

    def stage_two():
        fine.process_device(mid.data_ptr(), n1, n1, out.data_ptr(), n2)

    def both():
        chan.process_device(x.data_ptr(), N_IN, mid.data_ptr(), n1)
        stage_two()

    runs = take_turns(stream, {"ddc": lambda: ddc.process_device(x.data_ptr(), N_IN, out.data_ptr(), n2), "chan_fine": both,
                               "fine_alone": stage_two}, rounds)
    for obj in (ddc, chan, fine):
        obj.close()
    res = {"input": "rs16", "input_samples_per_call": N_IN, "bands": bands, "total_decimation": dd, "targets": targets,
           "ddc": dict(decimation=dd, taps=td, steps=steps, **figures(runs["ddc"])),
           "chan_fine": dict(channels_of=m1, decimation=d1, taps=t1, channels=channels, fine_decimation=d2, fine_taps=t2, fine_steps=steps2,
                             **figures(runs["chan_fine"])),
           "fine_alone": figures(runs["fine_alone"]), "rounds": rounds, "calls_per_timing": REPS}
    res["ddc_over_chan_fine_time"] = res["ddc"]["ms_per_call"] / res["chan_fine"]["ms_per_call"]
    for name in ("ddc", "chan_fine"):
        res[name]["input_gsps"] = N_IN / (res[name]["ms_per_call"] * 1e-3) / 1e9
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fine_rate.json"))
    ap.add_argument("--rounds", type=int, default=20, help="rounds of 10 calls per side (20 for a figure that is quoted)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("fine_rate.py measures on the GPU: none is available (there is nothing to report without one)")
    from sdrainer_amd.csrc import build
    build.build()
    from sdrainer_amd import capi, synth

    stream = torch.cuda.Stream()
    res = {"device": torch.cuda.get_device_name(0),
           "timing": "device events around 10 back-to-back calls on one stream, behind a warm-up; the sides take turns; medians over the rounds",
           "not_measured": "other input formats and shapes, a bank behind the chain, the kernels' own times by a profiler (the figures hold the host's launch path), a second box (the box-to-box spread)"}
    with torch.cuda.stream(stream):
        a = res["against_eight_one_band_ddcs"] = against_eight_ddcs(capi, synth, stream, args.rounds)
        print(f"8 bands from 8 f32 streams, D=8 T=128, 2^19 samples each: sdr_fine {a['fine']['ms_per_call']:.4f} ms/call, eight sdr_ddc "
              f"{a['eight_ddcs']['ms_per_call']:.4f} ms/call: {a['fine_over_eight_ddcs_time']:.3f}x (allowed excess {a['allowed_excess']:.3f}, "
              f"within: {a['within_spread']})", flush=True)
        b = res["chain_against_one_ddc"] = chain_against_ddc(capi, synth, stream, args.rounds)
        print(f"2^24 rs16 samples, 8 bands, total decimation 256: sdr_ddc D=256 T=2048 {b['ddc']['ms_per_call']:.3f} ms/call, sdr_chan + sdr_fine "
              f"{b['chan_fine']['ms_per_call']:.3f} ms/call (fine alone {b['fine_alone']['ms_per_call']:.3f}): {b['ddc_over_chan_fine_time']:.2f}x",
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
