#!/usr/bin/env python3
"""What the impulse noise blanker costs (sdr_nb_*; csrc/k_nb.hip), measured on the GPU with device events as interleaved runs
in one process, and written as JSON.

2^24 input samples per call, cu8 and sc16, B = 256, W = 16, ratio_q4 = 192, hold = 3, in front of a down-converter of 8 bands
at D = 8, T = 64 (the README's shape) and D = 64, T = 512.  Three sides over the same input take turns: the DDC alone on the
raw samples, the blanker followed by the DDC on the blanked samples (one stream, no synchronisation between them), and the
blanker alone.  Per side the median time of a call (every kernel of the call, by device events around back-to-back calls;
not a profiler's kernel time).  The blanker's three passes read the input twice and write it once: those bytes at the HBM
rate a streaming kernel achieves are set against the blanker's time.  The input is a few LSB of noise with a full-scale
sample every 10 007 samples, so the gate kernel has impulses to blank; the blanked share is reported.

    python tools/nb_rate.py [--out profiles/nb_rate.json] [--calls 200]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from ddc_rate import BANDS, N_IN, format_of  # noqa: E402
from iqc_rate import HBM_ACHIEVABLE, take_turns  # noqa: E402

BLOCK, WINDOW, RATIO_Q4, HOLD = 256, 16, 192, 3
SHAPES = ((8, 64, "cu8"), (8, 64, "sc16"), (64, 512, "cu8"), (64, 512, "sc16"))
PULSE_EVERY = 10_007


def noisy_input(capi, fmt_name, seed):
    """[N_IN, 2] raw samples on the device: uniform noise of an eighth of the range, a full-scale sample every PULSE_EVERY."""
    import torch

    _, _, dtype = format_of(capi, fmt_name)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    info = torch.iinfo(dtype)
    mid, span = (info.min + info.max + 1) // 2, (info.max - info.min + 1) // 16
    x = torch.randint(mid - span, mid + span, (N_IN, 2), dtype=dtype, device="cuda", generator=g)
    x[::PULSE_EVERY] = info.max
    return x


def sides(capi, synth, stream, d, t, fmt_name, calls):
    import torch

    fmt, _, _ = format_of(capi, fmt_name)
    m = N_IN // d
    x = noisy_input(capi, fmt_name, 9)
    clean = torch.empty_like(x)
    out = torch.empty((BANDS, m, 2), dtype=torch.float32, device="cuda")
    taps = synth.lowpass_taps(d, t // d)
    steps = [(b - BANDS // 2) * 4000 + 500 for b in range(BANDS)]
    ddc = {name: capi.Ddc(d, taps, steps, in_format=fmt, max_in_samples=N_IN) for name in ("ddc", "nb_ddc")}
    nb = {name: capi.Nb(fmt, BLOCK, WINDOW, RATIO_Q4, HOLD, max_in_samples=N_IN) for name in ("nb_ddc", "nb")}
    for o in list(ddc.values()) + list(nb.values()):
        o.set_stream(stream.cuda_stream)

    def both():
        nb["nb_ddc"].process_device(x.data_ptr(), N_IN, clean.data_ptr())
        ddc["nb_ddc"].process_device(clean.data_ptr(), N_IN, out.data_ptr(), m)

    side = {"ddc": lambda: ddc["ddc"].process_device(x.data_ptr(), N_IN, out.data_ptr(), m), "nb_ddc": both,
            "nb": lambda: nb["nb"].process_device(x.data_ptr(), N_IN, clean.data_ptr())}
    res, rounds, reps = take_turns(stream, side, calls)
    stats = nb["nb"].read_stats()
    for o in list(ddc.values()) + list(nb.values()):
        o.close()
    in_bytes = N_IN * x.element_size() * 2
    moved = 3 * in_bytes  # the power pass reads, the gate pass reads and writes
    plain, chained, alone = res["ddc"]["ms_per_call"], res["nb_ddc"]["ms_per_call"], res["nb"]["ms_per_call"]
    res.update({"bands": BANDS, "decimation": d, "taps": t, "input": fmt_name, "input_samples_per_call": N_IN, "block": BLOCK, "window": WINDOW,
                "ratio_q4": RATIO_Q4, "hold": HOLD, "rounds": rounds, "calls_per_timing": reps, "nb_ddc_over_ddc_time": chained / plain,
                "nb_cost_ms_by_difference": chained - plain, "nb_alone_over_ddc_time": alone / plain, "bytes_moved_by_the_blanker": moved,
                "bytes_moved_at_achievable_hbm_ms": moved / HBM_ACHIEVABLE * 1e3, "nb_alone_share_of_achievable_hbm": moved / HBM_ACHIEVABLE * 1e3 / alone,
                "samples": stats["samples"], "impulses": stats["impulses"], "blanked": stats["blanked"],
                "blanked_share": stats["blanked"] / max(1, stats["samples"])})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nb_rate.json"))
    ap.add_argument("--calls", type=int, default=200, help="calls per figure (at least 200 for a figure that is quoted)")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("nb_rate.py measures on the GPU: none is available (there is nothing to report without one)")
    from sdrainer_amd.csrc import build
    build.build()
    from sdrainer_amd import capi, synth

    stream = torch.cuda.Stream()
    res = {"device": torch.cuda.get_device_name(0), "boxes": 1, "source_hash": build.source_hash(), "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE,
           "timing": "device events around 10 back-to-back calls on one stream, behind a warm-up; the sides take turns; medians",
           "not_measured": "each pass's own time by a profiler (the blanker is priced as a whole, launch boundaries included; an input of 32 or "
                           "64 MB that the power pass has just read may reach the gate pass from the caches and not from HBM), the other four "
                           "formats, other block and window sizes, hold = B, a channelizer or a bank behind the blanker, "
                           "sdr_nb_process_host, a second box (the box-to-box spread)",
           "shapes": []}
    with torch.cuda.stream(stream):
        for d, t, fmt_name in SHAPES:
            r = sides(capi, synth, stream, d, t, fmt_name, args.calls)
            res["shapes"].append(r)
            print(f"D={d} T={t} {fmt_name}: DDC {r['ddc']['ms_per_call']:.4f} ms/call, blanker + DDC {r['nb_ddc']['ms_per_call']:.4f} "
                  f"(x{r['nb_ddc_over_ddc_time']:.4f}), blanker alone {r['nb']['ms_per_call'] * 1e3:.1f} us; its bytes at 6.3 TB/s "
                  f"{r['bytes_moved_at_achievable_hbm_ms'] * 1e3:.1f} us ({r['nb_alone_share_of_achievable_hbm'] * 100:.0f} %); "
                  f"blanked share {r['blanked_share']:.2e}", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
