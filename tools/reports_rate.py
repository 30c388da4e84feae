"""What listener reports cost (sdr_enable_reports): one bank of BASELINE config 3's geometry (one 2 MS/s band, N = 16384, 256
listeners, 8192 frames per batch) on device-resident frames, the same steps with reports off and with reports on, in one
process - through the C ABI, with delivery (sdr_poll_reports, then sdr_poll) inside the timed region as bench.py has sdr_poll.
The two settings alternate, `--pairs` times (off, on, off, on ...): one JSON line per run, then one line with the medians and
their ratio.  The comparison is against the reports-off runs of the same process, never a target.  For k_listen_report's
per-launch time beside k_listen_gather's run it under `rocprofv3 --kernel-trace --stats -- python tools/reports_rate.py --pairs 1`.
    python tools/reports_rate.py                       (config 3, three pairs of 20 steps)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384, choices=[4096, 8192, 16384, 32768, 65536])
    ap.add_argument("--bands", type=int, default=1)
    ap.add_argument("--frames", type=int, default=8192, help="frames per batch and band")
    ap.add_argument("--listeners", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=3)
    a = ap.parse_args()
    import torch

    from sdrainer_amd import capi, synth

    n, rate, bands, frames = a.n, 2_000_000, a.bands, a.frames
    iq, bins, _ = synth.make_band_torch(frames, rate, n, a.listeners, seed=33, device="cuda", free_last_window=True)
    batch = iq.reshape(-1).repeat(bands).contiguous()  # [band][frame][2N]: every band the same frames
    bank = capi.Bank(rate, n, n_bands=bands, edge_width=synth.default_edge_width(n), max_batch_frames=frames, max_listeners=a.listeners,
                     max_peaks=1024)
    bank.set_stream(torch.cuda.current_stream().cuda_stream)
    for b in range(bands):
        for bn in bins:
            bank.attach(b, int(bn))
    bank.enable_results(True)
    bank.enable_reports(True)  # (the report blocks exist from here on: switching on and off allocates nothing)
    bank.enable_reports(False)
    torch.cuda.synchronize()
    delivered = {"reports": 0, "ticks_on": 0, "peaks": 0, "edges": 0}

    def drain(wait=False):
        while True:
            rep = bank.poll_reports(wait=wait)
            if rep is None:
                return
            r = bank.poll_counts(wait=wait)
            assert r is not None and r[0] == rep[0], "sdr_poll delivered another batch than sdr_poll_reports looked at"
            delivered["reports"] += rep[1].shape[0]
            delivered["ticks_on"] += int(rep[1]["ticks_on"].sum())
            delivered["peaks"] += r[2]
            delivered["edges"] += r[4]
            wait = False

    def step():
        bank.process_device(batch.data_ptr(), frames)
        drain()

    def run(on):
        bank.enable_reports(on)
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
        line = {"n": n, "bands": bands, "frames_per_batch": frames, "listeners": a.listeners, "reports": int(on), "steps": a.steps,
                "ms_per_step": 1e3 * dt / a.steps, "frames_per_s": fps, "frame_gsps": fps * n / 1e9,
                "delivered_per_step": {k: v / a.steps for k, v in delivered.items()}}
        print(json.dumps(line), flush=True)
        return fps

    off, on = [], []
    for _ in range(a.pairs):
        off.append(run(False))
        on.append(run(True))
    m_off, m_on = statistics.median(off), statistics.median(on)
    print(json.dumps({"summary": "medians", "pairs": a.pairs, "gsps_reports_off": m_off * n / 1e9, "gsps_reports_on": m_on * n / 1e9,
                      "on_over_off": m_on / m_off}), flush=True)
    bank.close()


if __name__ == "__main__":
    main()
