"""Which FFT kernel a batch reaches (sdrainer_amd/csrc/host/batch_plan.h: fft_choice, fft_kernel, fft_kernel_name) driven
without a GPU by tests/host/test_fft_kernel_choice.cpp: every kernel id over the product of block size, input format,
window, hop, batch length, listener slots and the SDR_FFT_R32 / SDR_FFT_FPW switches, against the launchers' former hand-on
chain written out in the test; the frames-per-workgroup rule at its boundaries; and no planned choice that a unit's launcher
refuses."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_fft_kernel_choice.cpp")


@pytest.mark.parametrize("sanitizer", [None, "address,undefined"])
def test_fft_kernel_choice(tmp_path, sanitizer):
    exe = str(tmp_path / "test_fft_kernel_choice")
    flags = [f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all"] if sanitizer else []
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC], capture_output=True, text=True)
    if sanitizer and cc.returncode != 0 and "sanitize" in cc.stderr and "error:" not in cc.stderr.replace("-Werror", ""):
        pytest.skip("this compiler has no -fsanitize=" + sanitizer)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.split() == ["kernels", "ok", "frames_per_wg", "ok", "plan", "ok"]
