"""An sdr_group's bookkeeping (sdrainer_amd/csrc/host/group.h: band routing, the frame count of a staged group call, the
merge and parking of the members' deliveries) driven without a GPU by tests/host/test_group.cpp: synthetic member
batches merged must equal, field by field, what one bank of all the bands delivers - under the sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_group.cpp")


@pytest.mark.parametrize("sanitizer", [None, "address,undefined"])
def test_group_bookkeeping(tmp_path, sanitizer):
    exe = str(tmp_path / "test_group")
    flags = [f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all"] if sanitizer else []
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"] + flags + ["-o", exe, SRC],
                        capture_output=True, text=True)
    if sanitizer and cc.returncode != 0 and "sanitize" in cc.stderr and "error:" not in cc.stderr.replace("-Werror", ""):
        pytest.skip("this compiler has no -fsanitize=" + sanitizer)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.split() == ["routing", "ok", "frames", "ok", "merge2", "ok", "merge3", "ok", "offsets", "ok", "bad_size", "ok",
                                  "would_block", "ok", "out_of_step", "ok", "poll_peaks", "ok"]
