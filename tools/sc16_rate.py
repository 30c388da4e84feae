"""Development aid: the end-to-end rate of sc16 input (sdr_process_device_sc16) against float32 input
(sdr_process_device), both resident in HBM, at BASELINE config 3 (one band, N = 16384, 256 listeners, 8192 frames per
batch: k_fft_r32) and config 5 geometry (8 bands, N = 8192, 16 listeners per band, 2048 frames: k_fft_psd<13>).

The two formats are timed in interleaved A/B pairs (the order alternates from pair to pair), each run on a fresh bank with
its listeners attached and bulk delivery on: every batch's results are polled, as bench.py's timed loop does.  The input
is the same signal for both formats: synth.make_band_torch quantised to int16 (noise over hundreds of LSBs), and its
float32(x) / 32767 for the float32 runs.  Prints one JSON line per run and one summary line per workload.

    python tools/sc16_rate.py [--workloads c3,c5] [--pairs 3] [--steps 20] [--warmup 5]

Under rocprofv3 --kernel-trace --stats, --pairs 1 --steps 4 --warmup 1 gives the FFT kernels' own times per format
(k_fft_r32 / k_fft_r32_sc16, k_fft_psd / k_fft_psd_sc16)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from sdrainer_amd import capi, synth  # noqa: E402

# name: (sample_rate, block_size, listeners per band, bands, frames per batch, free_last_window)
WORKLOADS = {"c3": (2_000_000, 16384, 256, 1, 8192, True), "c5": (2_000_000, 8192, 16, 8, 2048, False)}
SCALE = 3.0e5


def make_input(name):
    rate, n, tones, bands, frames, free_last = WORKLOADS[name]
    q = torch.empty((bands, frames, 2 * n), dtype=torch.int16, device="cuda")
    bins_all = []
    for b in range(bands):
        iq, bins, _ = synth.make_band_torch(frames, rate, n, tones, seed=5000 + 17 * b, device="cuda", free_last_window=free_last)
        q[b] = torch.clamp(torch.round(iq.double() * SCALE), -32768, 32767).to(torch.int16)
        bins_all.append(bins)
        del iq
    f = (q.float() / np.float32(32767.0)).contiguous()
    torch.cuda.synchronize()
    return q.contiguous(), f, bins_all


def run(name, fmt, q, f, bins_all, steps, warmup):
    rate, n, tones, bands, frames, _ = WORKLOADS[name]
    bank = capi.Bank(rate, n, n_bands=bands, max_listeners=tones, max_batch_frames=frames, max_peaks=1024)
    stream = torch.cuda.Stream()
    bank.set_stream(stream.cuda_stream)
    for b, bins in enumerate(bins_all):
        for x in bins:
            bank.attach(b, int(x))
    bank.enable_results(True)
    go = (lambda: bank.process_device_sc16(q.data_ptr(), frames)) if fmt == "sc16" else (lambda: bank.process_device(f.data_ptr(), frames))
    in_flight = 0

    def step():
        nonlocal in_flight
        go()
        in_flight += 1
        if in_flight > 2:
            bank.poll_counts(wait=True)
            in_flight -= 1

    for _ in range(warmup):
        step()
    bank.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    while in_flight:
        bank.poll_counts(wait=True)
        in_flight -= 1
    dt = time.perf_counter() - t0
    bank.close()
    return steps * frames * bands * n / dt / 1e9, dt / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,c5")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    for name in a.workloads.split(","):
        q, f, bins_all = make_input(name)
        got = {"float32": [], "sc16": []}
        for p in range(a.pairs):
            order = ("float32", "sc16") if p % 2 == 0 else ("sc16", "float32")
            for fmt in order:
                gs, ms = run(name, fmt, q, f, bins_all, a.steps, a.warmup)
                got[fmt].append(gs)
                print(json.dumps({"workload": name, "pair": p, "format": fmt, "gsamples_per_s": round(gs, 2), "ms_per_step": round(ms, 4)}), flush=True)
        summary = {k: round(float(np.median(v)), 2) for k, v in got.items()}
        print(json.dumps({"workload": name, "median_gsamples_per_s": summary,
                          "sc16_over_float32": round(summary["sc16"] / summary["float32"], 4)}), flush=True)
        del q, f
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
