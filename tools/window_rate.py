"""What a window on the frames costs (sdr_set_window): one bank, one device-resident stream, the same steps first without
a window and then with a periodic Hann table, in one process - through the C ABI, with delivery (sdr_poll) inside the timed
region as bench.py does.  Prints two JSON lines (window: "none" / "hann") with frames per second and the ratio of the second
to the first.  The comparison is against the unwindowed run of the same geometry in the same process, never a target.
N = 16384: without a window long batches run k_fft_r32, with one k_fft_psd_win<14> (host/batch_plan.h); SDR_FFT_R32=0 in the
environment puts the unwindowed run on k_fft_psd<14> too, which separates what the window costs from what losing k_fft_r32
costs (the switches are read when a bank is created: one process per setting).  For the FFT kernels' per-launch times run
it under `rocprofv3 --kernel-trace --stats -- python tools/window_rate.py ...`.
    python tools/window_rate.py --n 8192 --bands 8 --frames 2048 --listeners 16      (config 5's geometry, dense)
    python tools/window_rate.py --n 16384 --hop 4096
    python tools/window_rate.py --n 65536 --hop 8192"""
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
    ap.add_argument("--bands", type=int, default=1)
    ap.add_argument("--frames", type=int, default=0, help="frames per batch and band (default: 128 M samples of frames over the bands)")
    ap.add_argument("--listeners", type=int, default=256)
    ap.add_argument("--sc16", action="store_true", help="complex int16 input")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch

    from sdrainer_amd import capi, synth

    n, rate, bands = a.n, 2_000_000, a.bands
    hop = a.hop or n
    frames = a.frames or (128 << 20) // (n * bands)
    iq, bins, _ = synth.make_band_torch(frames - 1 + n // hop, rate, hop, a.listeners, seed=33, device="cuda", free_last_window=True)
    stream = iq.reshape(-1)
    if a.sc16:
        stream = torch.round(stream * (30000.0 / float(stream.abs().max()))).to(torch.int16)
    span = (frames - 1) * hop + n
    assert stream.numel() == 2 * span
    stream = stream.repeat(bands).contiguous()  # [band][span][2]: every band the same stream
    bank = capi.Bank(rate, n, n_bands=bands, edge_width=synth.default_edge_width(n), max_batch_frames=frames, max_listeners=a.listeners,
                     max_peaks=1024, hop=a.hop)
    bank.set_stream(torch.cuda.current_stream().cuda_stream)
    for b in range(bands):
        for bn in bins:
            bank.attach(b, int(bn) * (n // hop))
    bank.enable_results(True)
    torch.cuda.synchronize()
    if a.hop:
        call = bank.process_device_stream_sc16 if a.sc16 else bank.process_device_stream
        process = lambda: call(stream.data_ptr(), frames, span)
    else:
        call = bank.process_device_sc16 if a.sc16 else bank.process_device
        process = lambda: call(stream.data_ptr(), frames)
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
        process()
        drain()

    base = None
    for name, table in (("none", None), ("hann", synth.hann(n))):
        if table is not None:
            bank.set_window(table)
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
        fps = a.steps * frames * bands / dt
        base = base or fps
        print(json.dumps({"n": n, "hop": hop, "bands": bands, "format": "sc16" if a.sc16 else "f32", "window": name,
                          "fft_r32_switch": os.environ.get("SDR_FFT_R32", "unset"), "frames_per_batch": frames, "listeners": a.listeners,
                          "steps": a.steps, "ms_per_step": 1e3 * dt / a.steps, "frames_per_s": fps, "frame_gsps": fps * n / 1e9,
                          "over_no_window": fps / base, "delivered_per_step": {k: v / a.steps for k, v in delivered.items()}}), flush=True)
    bank.close()


if __name__ == "__main__":
    main()
