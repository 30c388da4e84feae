"""The delivery state machine with a report block (sdrainer_amd/csrc/host/delivery.h: sdr_poll_reports' peek beside publish,
park and deliver) driven without a GPU by tests/host/test_delivery_reports.cpp: fake events, blocks and report blocks filled
per batch - ordering, the inactive slots left out, the refusal of a small buffer and its retry, parked batches keeping their
reports, the deferred listen half, the end of graph mode.  A stand-alone program, built plain and with the sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_delivery_reports.cpp")


@pytest.mark.parametrize("sanitizer", [None, "address,undefined"])
def test_delivery_reports(tmp_path, sanitizer):
    exe = str(tmp_path / "test_delivery_reports")
    flags = [f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all"] if sanitizer else []
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread"] + flags + ["-o", exe, SRC], capture_output=True, text=True)
    if sanitizer and cc.returncode != 0 and "sanitize" in cc.stderr and "error:" not in cc.stderr.replace("-Werror", ""):
        pytest.skip("this compiler has no -fsanitize=" + sanitizer)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.split() == ["order", "ok", "park", "ok", "deferred", "ok", "graph", "ok"]
