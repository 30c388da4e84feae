"""The delivery state machine with a row block (sdrainer_amd/csrc/host/delivery.h: sdr_poll_rows' peek beside publish, park
and deliver) driven without a GPU by tests/host/test_delivery_rows.cpp: fake events, blocks and row blocks stamped per
batch - ordering, the refusal of a small buffer and its retry, parked batches keeping their rows, the deferred listen half,
the end of graph mode, and a consumer thread beside the producer.  A stand-alone program, built with the sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_delivery_rows.cpp")


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_delivery_rows(tmp_path, sanitizer):
    exe = str(tmp_path / "test_delivery_rows")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", f"-fsanitize={sanitizer}",
                         "-fno-sanitize-recover=all", "-o", exe, SRC], capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr and "error:" not in cc.stderr.replace("-Werror", ""):
        pytest.skip("this compiler has no -fsanitize=" + sanitizer)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ThreadSanitizer" not in run.stderr and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.split() == ["order", "ok", "park", "ok", "deferred", "ok", "graph", "ok", "threads", "ok"]
