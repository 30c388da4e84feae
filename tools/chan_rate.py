#!/usr/bin/env python3
"""What the polyphase channelizer costs (sdr_chan_*, csrc/k_chan.hip) against the down-converter producing the same bands
(sdr_ddc_*, steps c L / M, the same decimation and taps) from the same input, measured on the GPU with device events as
interleaved pairs in one run, and written as JSON.

Pairs: M = 64 (all 64 channels), D = 32, T = 512 with cu8 and with rs16 input; M = 8 (all 8 channels), D = 8, T = 64 with
cu8 input (the README's DDC shape).  2^24 input samples per call.  Per side: ms per call (the kernel and the small carry
kernel behind it, by device events around back-to-back calls, not a profiler's kernel time), input GS/s, and the bytes the
algorithm needs (the input once, the outputs once) over the time, against the HBM peak.

    python tools/chan_rate.py [--out profiles/chan_rate.json] [--calls 200]
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

from ddc_rate import HBM_PEAK, N_IN, format_of, random_input, timed  # noqa: E402

PAIRS = ((64, 32, 512, "cu8"), (64, 32, 512, "rs16"), (8, 8, 64, "cu8"))
L = 65536


def pair(capi, synth, stream, m, d, t, fmt_name, calls):
    """Interleaved timings of the channelizer and of the DDC with one band per channel: the same input, D, taps and outputs."""
    import torch

    fmt, values, _ = format_of(capi, fmt_name)
    k = N_IN // d
    x = random_input(capi, fmt_name, 5)
    out = torch.empty((m, k, 2), dtype=torch.float32, device="cuda")
    taps = synth.lowpass_taps(d, t // d)
    assert len(taps) == t
    steps = [c * L // m - (L if c * L // m > 32767 else 0) for c in range(m)]
    chan = capi.Chan(m, d, taps, None, in_format=fmt, max_in_samples=N_IN)
    ddc = capi.Ddc(d, taps, steps, in_format=fmt, max_in_samples=N_IN)
    chan.set_stream(stream.cuda_stream)
    ddc.set_stream(stream.cuda_stream)
    side = {"chan": lambda: chan.process_device(x.data_ptr(), N_IN, out.data_ptr(), k),
            "ddc": lambda: ddc.process_device(x.data_ptr(), N_IN, out.data_ptr(), k)}
    reps, pairs = 10, max(1, calls // 10)
    for fn in side.values():
        timed(stream, fn, 20)  # warm-up
    runs = {name: [] for name in side}
    for _ in range(pairs):
        for name, fn in side.items():
            runs[name].append(timed(stream, fn, reps))
    chan.close()
    ddc.close()
    med = {name: float(np.median(r)) for name, r in runs.items()}
    need = N_IN * x.element_size() * values + out.numel() * 4
    res = {"channels": m, "decimation": d, "taps": t, "input": fmt_name, "input_samples_per_call": N_IN, "pairs": pairs,
           "calls_per_timing": reps, "needed_bytes_per_call": need, "tile_outputs": capi.chan_tile_outputs(m, d, t),
           "float32_ops_per_output_time_chan": 4 * t + 10 * (m // 2) * (m.bit_length() - 1), "float32_ops_per_output_time_ddc": m * (4 * t + 6 * d),
           "ddc_over_chan_time": med["ddc"] / med["chan"]}
    for name in side:
        res[name] = {"ms_per_call": med[name] * 1e3, "input_gsps": N_IN / med[name] / 1e9, "share_of_hbm_peak": need / HBM_PEAK / med[name],
                     "min_ms": min(runs[name]) * 1e3, "max_ms": max(runs[name]) * 1e3, "runs_ms": [r * 1e3 for r in runs[name]]}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chan_rate.json"))
    ap.add_argument("--calls", type=int, default=200, help="calls per figure (at least 200 for a figure that is quoted)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("chan_rate.py measures on the GPU: none is available (there is nothing to report without one)")
    from sdrainer_amd.csrc import build
    build.build()
    from sdrainer_amd import capi, synth

    stream = torch.cuda.Stream()
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK,
           "timing": "device events around 10 back-to-back calls on one stream, behind a warm-up; channelizer and DDC alternate; medians",
           "not_measured": "the other input formats, other geometries, a channel subset, the chain with a bank behind the channelizer, "
                           "a second box (the box-to-box spread)",
           "pairs": []}
    with torch.cuda.stream(stream):
        for m, d, t, fmt_name in PAIRS:
            r = pair(capi, synth, stream, m, d, t, fmt_name, args.calls)
            res["pairs"].append(r)
            print(f"M={m} D={d} T={t} {fmt_name}: channelizer {r['chan']['ms_per_call']:.3f} ms/call ({r['chan']['input_gsps']:.2f} GS/s in, "
                  f"{r['chan']['share_of_hbm_peak'] * 100:.1f} % of HBM peak), DDC with {m} bands {r['ddc']['ms_per_call']:.3f} ms/call "
                  f"({r['ddc']['input_gsps']:.2f} GS/s in): {r['ddc_over_chan_time']:.2f}x", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
