"""bench.py --dump-outputs: what the last timed step computed, written as .npy files that two runs (or two builds) can be
compared by.  The clock run-in takes as many steps as fit into --settle-ms, and it runs on a bank of its own, so two runs
that differ only there must write the same bits; the delivered batch's index shows that the measured bank ran exactly
its run-in, the warmup and --steps steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUN_IN_STEPS = 16  # bench.py
FRAMES, STEPS, WARMUP = 512, 7, 3


def _bench(out_dir, settle_ms):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c2", "--frames", str(FRAMES),
                        "--steps", str(STEPS), "--warmup", str(WARMUP), "--settle-ms", str(settle_ms), "--no-cpu-baseline",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dumped_outputs_do_not_depend_on_the_run_in(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    res = _bench(a, 20)
    _bench(b, 200)
    assert res["steps"] == STEPS and res["ms_per_step"] > 0
    samples = res["config"]["samples_per_step_per_gpu"]
    # (ms_per_step is rounded to four decimals)
    assert res["ms_per_step"] == pytest.approx(1e3 * samples / (res["value"] * 1e6), rel=1e-3, abs=1e-4)

    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"batch.npy", "chunks.npy", "peaks.npy", "listeners.npy", "edges.npy", "runes.npy", "rune_frames.npy",
            "frame_records.npy", "spectrum.npy", "psd.npy", "spectrum_frames.npy"} <= set(names)
    assert sum(os.path.getsize(a / f) for f in names) <= 64_000_000
    for f in names:
        x, y = np.load(a / f), np.load(b / f)
        assert x.dtype in (np.float32, np.float64), f
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{f} differs between the two runs"

    batch_index, first_frame, n_frames = np.load(a / "batch.npy")
    assert batch_index == RUN_IN_STEPS + WARMUP + STEPS - 1 and first_frame == batch_index * FRAMES and n_frames == FRAMES
    assert np.load(a / "frame_records.npy").shape == (FRAMES, 1, 8)
    assert len(np.load(a / "runes.npy")) > 0 and len(np.load(a / "edges.npy")) > 0


def test_bench_refuses_zero_steps():
    """(no GPU: the arguments are checked before torch is imported)"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=60)
    assert p.returncode == 2 and "--steps must be at least 1" in p.stderr, p.stderr[-1000:]
