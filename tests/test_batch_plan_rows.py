"""The batch plan with waterfall rows (sdrainer_amd/csrc/host/batch_plan.h) driven without a GPU by
tests/host/test_batch_plan_rows.cpp: rows off gives the plan a bank had before rows existed, stage by stage; rows on adds
exactly one stage, on the peaks stream behind the cumulate step, for the batches that complete a cumulation."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_batch_plan_rows.cpp")


@pytest.mark.parametrize("sanitizer", [None, "address,undefined"])
def test_batch_plan_rows(tmp_path, sanitizer):
    exe = str(tmp_path / "test_batch_plan_rows")
    flags = [f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all"] if sanitizer else []
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC], capture_output=True, text=True)
    if sanitizer and cc.returncode != 0 and "sanitize" in cc.stderr and "error:" not in cc.stderr.replace("-Werror", ""):
        pytest.skip("this compiler has no -fsanitize=" + sanitizer)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.split() == ["slots", "ok", "sweep", "ok"]
