"""Development aid: the end-to-end rate of 8-bit input (cs8 / cu8: sdr_process_device_iq8) against float32 and sc16 input,
all resident in HBM, at BASELINE config 3 (one band, N = 16384, 256 listeners, 8192 frames per batch: k_fft_r32*) and
config 5 geometry (8 bands, N = 8192, 16 listeners per band, 2048 frames: k_fft_psd*<13>).

The formats are timed in interleaved runs (the order rotates from round to round), each run on a fresh bank with its
listeners attached and bulk delivery on: every batch's results are polled, as bench.py's timed loop does.  The input is
the same signal for all formats: synth.make_band_torch with its noise raised to 2e-2 and quantised to 8 bits (x 120,
tests/iq8_tools.py), the float32 runs take the values those bytes stand for, the sc16 runs the bytes times 256.  Prints one
JSON line per run and one summary line per workload.

    python tools/iq8_rate.py [--workloads c3,c5] [--rounds 3] [--steps 20] [--warmup 5]
    python tools/iq8_rate.py --host [--rounds 3] [--steps 12]

--host: the PCIe-inclusive rate of the host-buffer boundary at config 3's geometry (2048-frame batches, as
tools/host_input_rate.py): sdr_push_iq8 + sdr_process_staged against sdr_push_iq and sdr_push_iq_sc16.

Under rocprofv3 --kernel-trace --stats, --rounds 1 --steps 4 --warmup 1 gives the FFT kernels' own times per format."""
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
FORMATS = ("float32", "sc16", "cs8", "cu8")
SCALE, SIGMA = 120.0, 2e-2


def make_input(name, frames=None):
    """{format: device tensor [bands, frames, 2N]} of one signal, and the tones' bins per band."""
    rate, n, tones, bands, batch, free_last = WORKLOADS[name]
    frames = frames or batch
    torch.manual_seed(1234)
    q = torch.empty((bands, frames, 2 * n), dtype=torch.int8, device="cuda")
    bins_all = []
    for b in range(bands):
        iq, bins, _ = synth.make_band_torch(frames, rate, n, tones, seed=5000 + 17 * b, device="cuda", free_last_window=free_last)
        iq += torch.randn(iq.shape, device="cuda", dtype=torch.float32) * SIGMA  # (the synth's own noise is 1e-3: silence in 8 bits)
        q[b] = torch.clamp(torch.round(iq.double() * SCALE), -128, 127).to(torch.int8)
        bins_all.append(bins)
        del iq
    data = {"cs8": q.contiguous(), "cu8": (q.to(torch.int16) + 128).to(torch.uint8).contiguous(),
            "sc16": (q.to(torch.int16) * 256).contiguous()}
    # float32 of the cs8 values: what the 8-bit runs compute with
    data["float32"] = (q.float() / np.float32(128.0)).contiguous()
    torch.cuda.synchronize()
    return data, bins_all


def make_bank(name, bins_all, frames=None):
    rate, n, tones, bands, batch, _ = WORKLOADS[name]
    bank = capi.Bank(rate, n, n_bands=bands, max_listeners=tones, max_batch_frames=frames or batch, max_peaks=1024)
    for b, bins in enumerate(bins_all):
        for x in bins:
            bank.attach(b, int(x))
    bank.enable_results(True)
    return bank


def run(name, fmt, data, bins_all, steps, warmup):
    rate, n, tones, bands, frames, _ = WORKLOADS[name]
    bank = make_bank(name, bins_all)
    stream = torch.cuda.Stream()
    bank.set_stream(stream.cuda_stream)
    ptr = data[fmt].data_ptr()
    go = {"float32": lambda: bank.process_device(ptr, frames), "sc16": lambda: bank.process_device_sc16(ptr, frames),
          "cs8": lambda: bank.process_device_iq8(ptr, frames, capi.IQ8_CS8), "cu8": lambda: bank.process_device_iq8(ptr, frames, capi.IQ8_CU8)}[fmt]
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


def run_host(fmt, host, bins_all, steps, frames):
    rate, n = WORKLOADS["c3"][:2]
    bank = make_bank("c3", bins_all, frames)
    x = host[fmt]
    push = {"float32": lambda: bank.push_iq(0, rate, x), "sc16": lambda: bank.push_iq_sc16(0, rate, x),
            "cs8": lambda: bank.push_iq8(0, rate, x, capi.IQ8_CS8), "cu8": lambda: bank.push_iq8(0, rate, x, capi.IQ8_CU8)}[fmt]

    def step():
        assert push() == 0
        assert bank.process_staged() == frames
        while bank.poll_counts(wait=False) is not None:
            pass

    for _ in range(2):
        step()
    bank.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    bank.sync()
    dt = time.perf_counter() - t0
    bank.close()
    return steps * frames * n / dt / 1e9, dt / steps * 1e3


def rounds_of(formats, rounds, one):
    got = {k: [] for k in formats}
    for r in range(rounds):
        for fmt in formats[r % len(formats):] + formats[:r % len(formats)]:
            gs, ms, extra = one(fmt)
            got[fmt].append(gs)
            print(json.dumps({**extra, "round": r, "format": fmt, "gsamples_per_s": round(gs, 3), "ms_per_step": round(ms, 4)}), flush=True)
    return {k: round(float(np.median(v)), 3) for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,c5")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    if a.host:
        frames = 2048
        data, bins_all = make_input("c3", frames)
        host = {k: v[0].cpu().numpy() for k, v in data.items()}
        del data
        torch.cuda.empty_cache()
        summary = rounds_of(FORMATS, a.rounds, lambda fmt: (*run_host(fmt, host, bins_all, a.steps, frames), {"workload": "c3-host", "frames": frames}))
        print(json.dumps({"workload": "c3-host", "median_gsamples_per_s": summary,
                          "over_float32": {k: round(v / summary["float32"], 3) for k, v in summary.items()}}), flush=True)
        return
    for name in a.workloads.split(","):
        data, bins_all = make_input(name)
        summary = rounds_of(FORMATS, a.rounds, lambda fmt: (*run(name, fmt, data, bins_all, a.steps, a.warmup), {"workload": name}))
        print(json.dumps({"workload": name, "median_gsamples_per_s": summary,
                          "over_float32": {k: round(v / summary["float32"], 4) for k, v in summary.items()}}), flush=True)
        del data
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
