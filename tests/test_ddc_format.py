"""The down-converter's input formats as the library's host code sees them (sdrainer_amd/csrc/host/ddc_format.h), driven
without a GPU by tests/host/test_ddc_format.cpp: over every int in [-2, 40] exactly {0..3, 16..19} are formats, with 8, 4, 2,
2, 4, 2, 1, 1 bytes per sample, their real flag and their complex base.  Built plain and under the address and
undefined-behaviour sanitizers, in the manner of tests/test_fft_kernel_choice.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_ddc_format.cpp")


@pytest.mark.parametrize("sanitizer", [None, "address,undefined"])
def test_ddc_format_table(tmp_path, sanitizer):
    exe = str(tmp_path / "test_ddc_format")
    flags = [f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all"] if sanitizer else []
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC], capture_output=True, text=True)
    if sanitizer and cc.returncode != 0 and "sanitize" in cc.stderr and "error:" not in cc.stderr.replace("-Werror", ""):
        pytest.skip("this compiler has no -fsanitize=" + sanitizer)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.split() == ["formats", "ok"]
