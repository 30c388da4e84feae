"""What waterfall rows cost (sdr_enable_rows): one bank of BASELINE config 3's geometry (one 2 MS/s band, N = 16384, 256
listeners, 8192 frames per batch) on device-resident frames, the same steps with rows off and with rows on, in one process -
through the C ABI, with delivery (sdr_poll_rows, then sdr_poll) inside the timed region as bench.py has sdr_poll.  The two
settings alternate, `--pairs` times (off, on, off, on ...): one JSON line per run, then one line with the medians and their
ratio.  The comparison is against the rows-off runs of the same process, never a target.  For k_cum_rows' per-launch time
run it under `rocprofv3 --kernel-trace --stats -- python tools/rows_rate.py --pairs 1`.
    python tools/rows_rate.py                       (config 3, 1024 columns, three pairs of 20 steps)
    python tools/rows_rate.py --columns 16384       (G = 1: the whole cumulation travels)"""
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
    ap.add_argument("--columns", type=int, default=1024)
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
    bank.enable_rows(a.columns)  # (the row blocks exist from here on: switching between 0 and a.columns allocates nothing)
    bank.enable_rows(0)
    torch.cuda.synchronize()
    delivered = {"rows": 0, "peaks": 0, "edges": 0}

    def drain(wait=False):
        while True:
            rows = bank.poll_rows(wait=wait)
            if rows is None:
                return
            r = bank.poll_counts(wait=wait)
            assert r is not None and r[0] == rows[0], "sdr_poll delivered another batch than sdr_poll_rows looked at"
            delivered["rows"] += rows[1].shape[0]
            delivered["peaks"] += r[2]
            delivered["edges"] += r[4]
            wait = False

    def step():
        bank.process_device(batch.data_ptr(), frames)
        drain()

    def run(columns):
        bank.enable_rows(columns)
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
        line = {"n": n, "bands": bands, "frames_per_batch": frames, "listeners": a.listeners, "rows": columns, "steps": a.steps,
                "ms_per_step": 1e3 * dt / a.steps, "frames_per_s": fps, "frame_gsps": fps * n / 1e9,
                "delivered_per_step": {k: v / a.steps for k, v in delivered.items()}}
        print(json.dumps(line), flush=True)
        return fps

    off, on = [], []
    for _ in range(a.pairs):
        off.append(run(0))
        on.append(run(a.columns))
    m_off, m_on = statistics.median(off), statistics.median(on)
    print(json.dumps({"summary": "medians", "pairs": a.pairs, "columns": a.columns, "gsps_rows_off": m_off * n / 1e9, "gsps_rows_on": m_on * n / 1e9,
                      "on_over_off": m_on / m_off}), flush=True)
    bank.close()


if __name__ == "__main__":
    main()
