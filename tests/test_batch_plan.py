"""The batch plan (sdrainer_amd/csrc/host/batch_plan.h: the environment's switches, the stream of every kernel, the FFT
kernel, the noise path, the bound and its refinement, the slot and chunk counts, the order of the stages) driven without a GPU by
tests/host/test_batch_plan.cpp: every rule pinned where it switches, every switch forced, invariants over a sweep -
under the sanitizers, and with the -DSDR_DIAG overrides compiled in."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_batch_plan.cpp")


@pytest.mark.parametrize("sanitizer, defines", [(None, []), ("address,undefined", []), ("address,undefined", ["-DSDR_DIAG"])])
def test_batch_plan(tmp_path, sanitizer, defines):
    exe = str(tmp_path / "test_batch_plan")
    flags = [f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all"] if sanitizer else []
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + defines + ["-o", exe, SRC],
                        capture_output=True, text=True)
    if sanitizer and cc.returncode != 0 and "sanitize" in cc.stderr and "error:" not in cc.stderr.replace("-Werror", ""):
        pytest.skip("this compiler has no -fsanitize=" + sanitizer)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.split() == ["switches", "ok", "fft", "ok", "bound", "ok", "parts", "ok", "gather", "ok", "refine", "ok", "counts", "ok",
                                  "forced", "ok", "order", "ok", "sweep", "ok"]
