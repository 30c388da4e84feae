"""The CUs k_fft_r32's grid leaves to the other streams' kernels (host/batch_plan.h fft_reserve_cus, SDR_FFT_RESERVE),
without a GPU: tests/host/test_batch_plan_reserve.cpp pins the rule at its boundaries, its clamp, the forced switch and
capture against eager."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")


def test_batch_plan_reserve(tmp_path):
    exe = str(tmp_path / "test_batch_plan_reserve")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                         os.path.join(HOST, "test_batch_plan_reserve.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.split() == ["plan", "ok"]
