"""Throughput with overlapped frames (sdr_config.hop < block_size, sdr_process_device_stream): a config-3-shaped workload -
2 MS/s, 256 listeners, a batch of about 128 M samples OF FRAMES (8192 frames at N = 16384, 2048 at 65536) read from one
device-resident stream of (frames - 1) * hop + N samples - through the C ABI, with delivery (sdr_poll) inside the timed
region as bench.py does.  Prints one JSON line: frames per second, and input GS/s counted in NEW samples (frames * hop per
batch: what a ring would have received in that time).  --hop 0 (= N) is the dense baseline on the same entry point.  For the
FFT kernels' per-launch times run it under `rocprofv3 --kernel-trace --stats -- python tools/overlap_rate.py ...`.
    python tools/overlap_rate.py --n 16384 --hop 4096 --steps 20 --warmup 3"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384, choices=[4096, 8192, 16384, 32768, 65536])
    ap.add_argument("--hop", type=int, default=0, help="samples between frame starts (0: N, frames do not overlap)")
    ap.add_argument("--frames", type=int, default=0, help="frames per batch (default: 128 M samples of frames)")
    ap.add_argument("--listeners", type=int, default=256)
    ap.add_argument("--sc16", action="store_true", help="complex int16 input (sdr_process_device_stream_sc16)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch

    from sdrainer_amd import capi, synth

    n, rate = a.n, 2_000_000
    hop = a.hop or n
    frames = a.frames or (128 << 20) // n
    # one frame of the short transform per hop: flattened, a phase-continuous stream keyed per hop; bin i of the hop-point
    # spectrum is bin i * N / hop of the N-point one
    iq, bins, _ = synth.make_band_torch(frames - 1 + n // hop, rate, hop, a.listeners, seed=33, device="cuda", free_last_window=True)
    stream = iq.reshape(-1)
    if a.sc16:
        stream = torch.round(stream * (30000.0 / float(stream.abs().max()))).to(torch.int16)
    span = (frames - 1) * hop + n
    assert stream.numel() == 2 * span
    bank = capi.Bank(rate, n, edge_width=synth.default_edge_width(n), max_batch_frames=frames, max_listeners=a.listeners, max_peaks=1024,
                     hop=a.hop)
    bank.set_stream(torch.cuda.current_stream().cuda_stream)
    for bn in bins:
        bank.attach(0, int(bn) * (n // hop))
    bank.enable_results(True)
    torch.cuda.synchronize()
    process = bank.process_device_stream_sc16 if a.sc16 else bank.process_device_stream
    delivered = {"edges": 0, "runes": 0, "peaks": 0}

    def drain():
        while True:
            r = bank.poll_counts(wait=False)
            if r is None:
                return
            delivered["peaks"] += r[2]
            delivered["edges"] += r[4]
            delivered["runes"] += r[5]

    def step():
        process(stream.data_ptr(), frames, span)
        drain()

    for _ in range(a.warmup):
        step()
    bank.sync()
    drain()
    for k in delivered:
        delivered[k] = 0
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    bank.sync()
    drain()
    dt = time.perf_counter() - t0
    print(json.dumps({"n": n, "hop": hop, "format": "sc16" if a.sc16 else "f32", "frames_per_batch": frames, "listeners": a.listeners,
                      "steps": a.steps, "ms_per_step": 1e3 * dt / a.steps, "frames_per_s": a.steps * frames / dt,
                      "frame_gsps": a.steps * frames * n / dt / 1e9, "input_gsps": a.steps * frames * hop / dt / 1e9,
                      "delivered_per_step": {k: v / a.steps for k, v in delivered.items()}}))
    bank.close()


if __name__ == "__main__":
    main()
