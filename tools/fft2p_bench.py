"""Throughput at N = 32768 / 65536 (the two-phase FFT, k_fft_2p.hip): a config-3-shaped workload - 61 Hz bins (2 MS/s at
32768, 4 MS/s at 65536), 256 listeners, about 128 M samples per batch (4096 / 2048 frames) - through the C ABI, with
delivery (sdr_poll) inside the timed region as bench.py does.  Prints one JSON line.  For the two phases' kernel times run
it under `rocprofv3 --kernel-trace --stats -- python tools/fft2p_bench.py ...`; SDR_FFT2P_GROUP_MB=0 puts the whole batch
in one frame group (no Infinity-Cache-sized groups) for comparison.
    python tools/fft2p_bench.py --n 32768 --steps 20 --warmup 3"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768, choices=[32768, 65536])
    ap.add_argument("--frames", type=int, default=0, help="frames per batch (default: 128 M samples)")
    ap.add_argument("--listeners", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch

    from sdrainer_amd import capi, synth

    n = a.n
    rate = 2_000_000 * n // 32768
    frames = a.frames or (128 << 20) // n
    iq, bins, _ = synth.make_band_torch(frames, rate, n, a.listeners, seed=33, device="cuda")
    bank = capi.Bank(rate, n, edge_width=synth.default_edge_width(n), max_batch_frames=frames, max_listeners=a.listeners, max_peaks=1024)
    bank.set_stream(torch.cuda.current_stream().cuda_stream)
    for bn in bins:
        bank.attach(0, int(bn))
    bank.enable_results(True)
    torch.cuda.synchronize()

    def step():
        bank.process_device(iq.data_ptr(), frames)
        while bank.poll(wait=False) is not None:
            pass

    for _ in range(a.warmup):
        step()
    bank.sync()
    while bank.poll(wait=False) is not None:
        pass
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    bank.sync()
    while bank.poll(wait=False) is not None:
        pass
    dt = time.perf_counter() - t0
    print(json.dumps({"n": n, "frames_per_batch": frames, "listeners": a.listeners, "steps": a.steps,
                      "group_mb": os.environ.get("SDR_FFT2P_GROUP_MB", "default"),
                      "ms_per_step": 1e3 * dt / a.steps, "gsps": a.steps * frames * n / dt / 1e9}))
    bank.close()


if __name__ == "__main__":
    main()
