#!/usr/bin/env python3
"""What the IQ correction and the raw stream's sums cost (sdr_iq_*_set_correction, sdr_iq_*_enable_sums; csrc/k_ddc_iqc.hip,
k_chan_iqc.hip, k_iq_sums.hip), measured on the GPU with device events as interleaved runs in one process, and written as JSON.

Down-converter, 8 bands, 2^24 input samples per call, cu8 and sc16, at D = 8, T = 64 (the README's shape) and D = 64, T = 512:
three objects over the same input take turns - plain, with a correction set, with the sums on.  Per side the median time of
a call (the kernel, the carry's kernel and, with the sums on, the two sums kernels, by device events around back-to-back
calls; not a profiler's kernel time).  The sums pass is priced by difference (sums on minus plain: its two kernels and
their boundaries) and set against the time to read the call's input once at the HBM rate a streaming kernel achieves.
Channelizer, M = 64 (all channels), D = 32, T = 512, cu8: plain against corrected.

    python tools/iqc_rate.py [--out profiles/iqc_rate.json] [--calls 200]
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

from ddc_rate import BANDS, N_IN, format_of, random_input, timed  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes/s: what a streaming float4 copy reaches on an MI355X (8.0e12 is the spec)
CORR = (0.0123, -0.0217, 1.0471, -0.0533)
DDC_SHAPES = ((8, 64, "cu8"), (8, 64, "sc16"), (64, 512, "cu8"), (64, 512, "sc16"))
CHAN_SHAPE = (64, 32, 512, "cu8")


def take_turns(stream, side, calls, between=None):
    """between: called behind the warm-up and behind every round, outside the timed windows."""
    reps, rounds = 10, max(1, calls // 10)
    for fn in side.values():
        timed(stream, fn, 20)  # warm-up
    runs = {name: [] for name in side}
    for _ in range(rounds):
        if between:
            between()
        for name, fn in side.items():
            runs[name].append(timed(stream, fn, reps))
    return {name: {"ms_per_call": float(np.median(r)) * 1e3, "min_ms": min(r) * 1e3, "max_ms": max(r) * 1e3, "runs_ms": [v * 1e3 for v in r]}
            for name, r in runs.items()}, rounds, reps


def ddc_sides(capi, synth, stream, d, t, fmt_name, calls):
    import torch

    fmt, _, _ = format_of(capi, fmt_name)
    m = N_IN // d
    x = random_input(capi, fmt_name, 5)
    out = torch.empty((BANDS, m, 2), dtype=torch.float32, device="cuda")
    taps = synth.lowpass_taps(d, t // d)
    steps = [(b - BANDS // 2) * 4000 + 500 for b in range(BANDS)]
    objs = {name: capi.Ddc(d, taps, steps, in_format=fmt, max_in_samples=N_IN) for name in ("plain", "corrected", "sums_on")}
    for o in objs.values():
        o.set_stream(stream.cuda_stream)
    objs["corrected"].set_iq_correction(CORR)
    objs["sums_on"].enable_iq_sums(True)
    side = {name: (lambda o=o: o.process_device(x.data_ptr(), N_IN, out.data_ptr(), m)) for name, o in objs.items()}
    # the sums are read in front of every round, as a receiver reads them: 2^32 samples are 256 of these calls, and a call
    # behind them would be skipped, not summed
    res, rounds, reps = take_turns(stream, side, calls, between=objs["sums_on"].read_iq_sums)
    summed = objs["sums_on"].read_iq_sums()
    for o in objs.values():
        o.close()
    in_bytes = N_IN * x.element_size() * 2
    plain, sums = res["plain"]["ms_per_call"], res["sums_on"]["ms_per_call"]
    res.update({"bands": BANDS, "decimation": d, "taps": t, "input": fmt_name, "input_samples_per_call": N_IN, "rounds": rounds,
                "calls_per_timing": reps, "corrected_over_plain_time": res["corrected"]["ms_per_call"] / plain, "sums_on_over_plain_time": sums / plain,
                "sums_pass_ms_by_difference": sums - plain, "input_bytes_per_call": in_bytes,
                "input_read_once_at_achievable_hbm_ms": in_bytes / HBM_ACHIEVABLE * 1e3,
                "sums_pass_share_of_achievable_hbm": (in_bytes / HBM_ACHIEVABLE * 1e3) / (sums - plain) if sums > plain else None,
                "samples_summed": summed["n"], "samples_skipped": summed["skipped"]})
    return res


def chan_sides(capi, synth, stream, m, d, t, fmt_name, calls):
    import torch

    fmt, _, _ = format_of(capi, fmt_name)
    k = N_IN // d
    x = random_input(capi, fmt_name, 5)
    out = torch.empty((m, k, 2), dtype=torch.float32, device="cuda")
    taps = synth.lowpass_taps(d, t // d)
    objs = {name: capi.Chan(m, d, taps, None, in_format=fmt, max_in_samples=N_IN) for name in ("plain", "corrected")}
    for o in objs.values():
        o.set_stream(stream.cuda_stream)
    objs["corrected"].set_iq_correction(CORR)
    side = {name: (lambda o=o: o.process_device(x.data_ptr(), N_IN, out.data_ptr(), k)) for name, o in objs.items()}
    res, rounds, reps = take_turns(stream, side, calls)
    for o in objs.values():
        o.close()
    res.update({"channels": m, "decimation": d, "taps": t, "input": fmt_name, "input_samples_per_call": N_IN, "rounds": rounds,
                "calls_per_timing": reps, "corrected_over_plain_time": res["corrected"]["ms_per_call"] / res["plain"]["ms_per_call"]})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iqc_rate.json"))
    ap.add_argument("--calls", type=int, default=200, help="calls per figure (at least 200 for a figure that is quoted)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("iqc_rate.py measures on the GPU: none is available (there is nothing to report without one)")
    from sdrainer_amd.csrc import build
    build.build()
    from sdrainer_amd import capi, synth

    stream = torch.cuda.Stream()
    res = {"device": torch.cuda.get_device_name(0), "boxes": 1, "source_hash": build.source_hash(), "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
           "timing": "device events around 10 back-to-back calls on one stream, behind a warm-up; the sides take turns; medians",
           "not_measured": "the sums kernel's own time by a profiler (it is priced by difference, boundaries included, and its input has just "
                           "been read by the main kernel, so part of it may come from the caches and not from HBM), float32 and cs8 input, "
                           "other geometries, the chain with a bank behind the corrected DDC, a second box (the box-to-box spread)",
           "ddc": [], "chan": None}
    with torch.cuda.stream(stream):
        for d, t, fmt_name in DDC_SHAPES:
            r = ddc_sides(capi, synth, stream, d, t, fmt_name, args.calls)
            res["ddc"].append(r)
            share = r["sums_pass_share_of_achievable_hbm"]
            print(f"DDC D={d} T={t} {fmt_name}: plain {r['plain']['ms_per_call']:.4f} ms/call, corrected x{r['corrected_over_plain_time']:.4f}, "
                  f"sums on x{r['sums_on_over_plain_time']:.4f} (the pass {r['sums_pass_ms_by_difference'] * 1e3:.1f} us, input once at 6.3 TB/s "
                  f"{r['input_read_once_at_achievable_hbm_ms'] * 1e3:.1f} us" + (f", {share * 100:.0f} %)" if share else ")"), flush=True)
        m, d, t, fmt_name = CHAN_SHAPE
        r = chan_sides(capi, synth, stream, m, d, t, fmt_name, args.calls)
        res["chan"] = r
        print(f"channelizer M={m} D={d} T={t} {fmt_name}: plain {r['plain']['ms_per_call']:.4f} ms/call, corrected x{r['corrected_over_plain_time']:.4f}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
