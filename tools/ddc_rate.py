#!/usr/bin/env python3
"""What the down-converter costs (sdr_ddc_*, csrc/k_ddc.hip), measured on the GPU with device events and written as JSON.

(a) The DDC alone: cu8 and float32 input, 8 bands, (D, T) = (8, 64) and (64, 512), 2^24 input samples per call, CALLS calls
    back to back on one stream behind a warm-up.  Per configuration: input MS/s; the bytes the algorithm needs (the input
    once, the outputs once) over the time, against the HBM peak; its 4 T / D n_bands float32 operations per input sample
    against the float32 vector peak; and which of the two bounds it.  The time is the calls' time by device events (the
    DDC kernel and the small carry kernel behind it), not a profiler's kernel time.
(b) The chain: the DDC (cu8, D = 8, T = 64) plus a bank of 8 bands at N = 16384 on the same stream, against the same bank
    fed the precomputed DDC output through sdr_process_device_stream - as interleaved pairs in one run.

(c) With --real, instead of (a) and (b): a real format against the complex format of the same sample type (rs16 against
    sc16, ru8 against cu8), the same number of input samples per call, as interleaved pairs in one run - the real form reads
    half the bytes and mixes with im = +0.0f, everything behind the mix is the same kernel body.

    python tools/ddc_rate.py [--out profiles/ddc_rate.json] [--calls 200]
    python tools/ddc_rate.py --real [--out profiles/ddc_real_rate.json] [--calls 200]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12     # bytes/s, spec (6.3e12 measured with a float4 copy)
FP32_PEAK = 157.3e12  # float32 operations/s on the vector ALU, spec (a fused multiply-add counted as two)
N_IN = 1 << 24
BANDS = 8


def timed(stream, fn, reps):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(reps):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def format_of(capi, fmt_name):
    """(in_format, values per sample, torch dtype) of a format by name: f32 sc16 cs8 cu8, and rf32 rs16 rs8 ru8 real."""
    import torch

    fmt = getattr(capi, "DDC_" + fmt_name.upper())
    dtype = {capi.DDC_F32: torch.float32, capi.DDC_SC16: torch.int16, capi.DDC_CS8: torch.int8, capi.DDC_CU8: torch.uint8}[fmt & ~capi.DDC_REAL]
    return fmt, 1 if fmt & capi.DDC_REAL else 2, dtype


def random_input(capi, fmt_name, seed):
    """N_IN raw samples of the format in device memory, over the format's whole range: [N_IN, 2] complex, [N_IN] real."""
    import torch

    _, values, dtype = format_of(capi, fmt_name)
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    shape = (N_IN, 2) if values == 2 else (N_IN,)
    if dtype == torch.float32:
        return torch.rand(shape, dtype=torch.float32, device="cuda", generator=g) * 2 - 1
    info = torch.iinfo(dtype)
    return torch.randint(info.min, info.max + 1, shape, dtype=dtype, device="cuda", generator=g)


def ddc_alone(capi, synth, stream, fmt_name, d, t, calls):
    import torch

    fmt, values, _ = format_of(capi, fmt_name)
    x = random_input(capi, fmt_name, 1)
    m = N_IN // d
    out = torch.empty((BANDS, m, 2), dtype=torch.float32, device="cuda")
    steps = [(-28000 + 8000 * b) for b in range(BANDS)]
    ddc = capi.Ddc(d, synth.lowpass_taps(d, t // d), steps, in_format=fmt, max_in_samples=N_IN)
    ddc.set_stream(stream.cuda_stream)
    call = lambda: ddc.process_device(x.data_ptr(), N_IN, out.data_ptr(), m)
    timed(stream, call, 20)  # warm-up
    runs = [timed(stream, call, calls // 4) for _ in range(4)]
    ddc.close()
    s = float(np.median(runs))
    in_bytes = N_IN * x.element_size() * values
    need_bytes = in_bytes + out.numel() * 4
    flops = 4.0 * t / d * BANDS * N_IN
    t_mem, t_alu = need_bytes / HBM_PEAK, flops / FP32_PEAK
    return {
        "input": fmt_name, "bands": BANDS, "decimation": d, "taps": t, "input_samples_per_call": N_IN, "calls": 4 * (calls // 4),
        "seconds_per_call": s, "seconds_per_call_runs": runs, "input_msps": N_IN / s / 1e6,
        "needed_bytes_per_call": need_bytes, "needed_bytes_per_s": need_bytes / s, "share_of_hbm_peak": t_mem / s,
        "float32_ops_per_call": flops, "float32_ops_per_s": flops / s, "share_of_fp32_vector_peak": t_alu / s,
        "bound": "float32 vector peak" if t_alu > t_mem else "HBM",
    }


REAL_PAIRS = (("rs16", "sc16", 8, 64), ("rs16", "sc16", 64, 512), ("rs16", "sc16", 256, 2048), ("ru8", "cu8", 8, 64))


def real_pair(capi, synth, stream, real_name, complex_name, d, t, calls):
    """Interleaved timings of one real format and its complex counterpart: the same geometry, bands and samples per call."""
    import torch

    m = N_IN // d
    out = torch.empty((BANDS, m, 2), dtype=torch.float32, device="cuda")
    steps = [(-28000 + 8000 * b) for b in range(BANDS)]
    taps = synth.lowpass_taps(d, t // d)
    side = {}
    for name in (real_name, complex_name):
        x = random_input(capi, name, 3)
        ddc = capi.Ddc(d, taps, steps, in_format=format_of(capi, name)[0], max_in_samples=N_IN)
        ddc.set_stream(stream.cuda_stream)
        side[name] = (ddc, x, lambda ddc=ddc, x=x: ddc.process_device(x.data_ptr(), N_IN, out.data_ptr(), m))
    reps, pairs = 10, max(1, calls // 10)
    for name in side:
        timed(stream, side[name][2], 20)  # warm-up
    runs = {name: [] for name in side}
    for _ in range(pairs):
        for name in side:
            runs[name].append(timed(stream, side[name][2], reps))
    for ddc, _, _ in side.values():
        ddc.close()
    med = {name: float(np.median(r)) for name, r in runs.items()}
    return {
        "real": real_name, "complex": complex_name, "bands": BANDS, "decimation": d, "taps": t, "input_samples_per_call": N_IN,
        "pairs": pairs, "calls_per_timing": reps,
        "real_seconds_per_call": med[real_name], "complex_seconds_per_call": med[complex_name],
        "real_input_msps": N_IN / med[real_name] / 1e6, "complex_input_msps": N_IN / med[complex_name] / 1e6,
        "real_input_bytes_per_call": side[real_name][1].numel() * side[real_name][1].element_size(),
        "complex_input_bytes_per_call": side[complex_name][1].numel() * side[complex_name][1].element_size(),
        "real_over_complex_time": med[real_name] / med[complex_name],
        "real_runs": runs[real_name], "complex_runs": runs[complex_name],
    }


def chain(capi, synth, stream, calls):
    """Pairs of (DDC + bank, the same bank on precomputed DDC output), alternating, `reps` calls per timing."""
    import torch

    d, t, n, rate = 8, 64, 16384, 2_000_000
    m = N_IN // d
    frames = m // n
    g = torch.Generator(device="cuda")
    g.manual_seed(2)
    # noise plus one strong carrier per band would not change the launches; plain noise bytes keep the tool simple
    x = torch.randint(96, 160, (N_IN, 2), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty((BANDS, m, 2), dtype=torch.float32, device="cuda")
    steps = [(-28000 + 8000 * b) for b in range(BANDS)]
    ddc = capi.Ddc(d, synth.lowpass_taps(d, t // d), steps, in_format=capi.DDC_CU8, max_in_samples=N_IN)
    ddc.set_stream(stream.cuda_stream)
    banks = []
    for _ in range(2):
        bank = capi.Bank(rate, n, n_bands=BANDS, max_batch_frames=frames, max_listeners=16, max_peaks=256)
        bank.set_stream(stream.cuda_stream)
        for b in range(BANDS):
            for l in range(16):
                bank.attach(b, 2000 + 700 * l)
        banks.append(bank)

    def with_ddc():
        ddc.process_device(x.data_ptr(), N_IN, out.data_ptr(), m)
        banks[0].process_device_stream(out.data_ptr(), frames, m)

    def bank_only():
        banks[1].process_device_stream(out.data_ptr(), frames, m)

    with_ddc()
    stream.synchronize()
    reps, pairs = 10, max(1, calls // 10)
    timed(stream, with_ddc, reps)
    timed(stream, bank_only, reps)
    a, b = [], []
    for _ in range(pairs):
        a.append(timed(stream, with_ddc, reps))
        b.append(timed(stream, bank_only, reps))
    for bank in banks:
        bank.sync()
        bank.close()
    ddc.close()
    ma, mb = float(np.median(a)), float(np.median(b))
    return {
        "input": "cu8", "bands": BANDS, "decimation": d, "taps": t, "block_size": n, "frames_per_band_per_call": frames,
        "listeners_per_band": 16, "input_samples_per_call": N_IN, "pairs": pairs, "calls_per_timing": reps,
        "ddc_and_bank_seconds_per_call": ma, "bank_alone_seconds_per_call": mb, "ddc_share_of_chain": (ma - mb) / ma,
        "ddc_and_bank_input_msps": N_IN / ma / 1e6, "bank_alone_narrow_msps_all_bands": BANDS * m / mb / 1e6,
        "ddc_and_bank_runs": a, "bank_alone_runs": b,
    }


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--real", action="store_true", help="measure the real formats against their complex counterparts, in pairs")
    ap.add_argument("--out", default=None, help="default: profiles/ddc_rate.json, with --real profiles/ddc_real_rate.json")
    ap.add_argument("--calls", type=int, default=200, help="calls per figure (at least 200 for a figure that is quoted)")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "ddc_real_rate.json" if args.real else "ddc_rate.json")
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("ddc_rate.py measures on the GPU: none is available (there is nothing to report without one)")
    from sdrainer_amd.csrc import build
    build.build()
    from sdrainer_amd import capi, synth

    stream = torch.cuda.Stream()
    res = {"device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "fp32_vector_peak_ops_per_s": FP32_PEAK}
    with torch.cuda.stream(stream):
        if args.real:
            res["timing"] = "device events around 10 back-to-back calls on one stream, behind a warm-up; real and complex alternate; medians"
            res["real_pairs"] = []
            for real_name, complex_name, d, t in REAL_PAIRS:
                r = real_pair(capi, synth, stream, real_name, complex_name, d, t, args.calls)
                res["real_pairs"].append(r)
                print(f"{real_name} vs {complex_name} D={d} T={t}: {r['real_seconds_per_call'] * 1e3:.3f} / {r['complex_seconds_per_call'] * 1e3:.3f} ms/call, "
                      f"{r['real_input_msps']:.0f} / {r['complex_input_msps']:.0f} MS/s in, time ratio {r['real_over_complex_time']:.3f}", flush=True)
        else:
            res.update({"timing": "device events around back-to-back calls on one stream, behind a warm-up; medians", "ddc_alone": [], "chain": None})
            for fmt in ("cu8", "f32"):
                for d, t in ((8, 64), (64, 512)):
                    r = ddc_alone(capi, synth, stream, fmt, d, t, args.calls)
                    res["ddc_alone"].append(r)
                    print(f"ddc alone {fmt} D={d} T={t}: {r['seconds_per_call'] * 1e3:.3f} ms/call, {r['input_msps']:.0f} MS/s in, "
                          f"{r['share_of_hbm_peak'] * 100:.1f} % of HBM peak, {r['share_of_fp32_vector_peak'] * 100:.1f} % of fp32 vector peak "
                          f"(bound: {r['bound']})", flush=True)
            res["chain"] = c = chain(capi, synth, stream, args.calls)
            print(f"chain: ddc + bank {c['ddc_and_bank_seconds_per_call'] * 1e3:.3f} ms/call, bank alone {c['bank_alone_seconds_per_call'] * 1e3:.3f} ms/call",
                  flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
