"""The batch plan with listener reports (sdrainer_amd/csrc/host/batch_plan.h) driven without a GPU by
tests/host/test_batch_plan_reports.cpp: reports off gives the plan a bank had before reports existed, stage by stage, over the
sweep the rows test uses; reports on adds exactly the report launches, on the decode stage's stream, for the batches that have
listener slots."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_batch_plan_reports.cpp")


@pytest.mark.parametrize("sanitizer", [None, "address,undefined"])
def test_batch_plan_reports(tmp_path, sanitizer):
    exe = str(tmp_path / "test_batch_plan_reports")
    flags = [f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all"] if sanitizer else []
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC], capture_output=True, text=True)
    if sanitizer and cc.returncode != 0 and "sanitize" in cc.stderr and "error:" not in cc.stderr.replace("-Werror", ""):
        pytest.skip("this compiler has no -fsanitize=" + sanitizer)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.split() == ["slots", "ok", "sweep", "ok"]
