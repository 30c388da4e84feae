"""sdr_fine_tune's integer rule as the library's host code has it (sdrainer_amd/csrc/host/fine_tune.h), walked without a GPU
and without the library by the stand-alone program tests/host/fine_tune_main.cpp: over every legal channelizer geometry the
result equals a search for the nearest channel centre, ties to the even channel, the step 32768 wrapped; refusals leave the
outputs alone, at the ends of int64_t too.  Built plain and under the address and undefined-behaviour sanitizers, in the
manner of tests/test_ddc_format.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "fine_tune_main.cpp")


@pytest.mark.parametrize("sanitizer", [None, "address,undefined"])
def test_fine_tune_rule(tmp_path, sanitizer):
    exe = str(tmp_path / "fine_tune_main")
    flags = [f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all"] if sanitizer else []
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC], capture_output=True, text=True)
    if sanitizer and cc.returncode != 0 and "sanitize" in cc.stderr and "error:" not in cc.stderr.replace("-Werror", ""):
        pytest.skip("this compiler has no -fsanitize=" + sanitizer)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.split() == ["tune", "ok"]
