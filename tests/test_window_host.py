"""A window on the frames (sdr_set_window) without a GPU: the symbols, synth.hann, the batch plan's rule for a windowed
bank (tests/host/test_batch_plan_window.cpp), and the oracle-only half of the demonstration the feature exists for, so
that its input is pinned where no GPU is needed (tests/test_window_gpu.py runs the bank against it).

The demonstration (192 kS/s, N = 4096, hop = 1024, one listener on bin 2600): a weak station exactly on bin 2600 keys a
call sign; a neighbour 50 dB stronger sits half-way between two bins, 11.5 bins below.  Under the rectangular window the
neighbour's leakage (falling as 1 / (pi * distance in bins)) buries the weak station: FindPeaks sees the two as one run
and the listener decodes nothing of the call sign.  Under a Hann window the two are two peaks and the call sign is read."""
import os
import re
import subprocess

import numpy as np
import pytest

from parity_tools import DEMO, check_demo_oracle, demo_oracle, demo_stream, merged_runs, windowed
from sdrainer_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
NEW_SYMBOLS = ["sdr_set_window", "sdr_group_set_window"]


@pytest.fixture(scope="module")
def lib():
    from sdrainer_amd.csrc import build
    return build.build()


def test_symbols_in_library_header_and_binding(lib):
    from sdrainer_amd import capi
    dyn = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "sdrainer_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in exported, f"{name} is not exported by the library"
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in the header"
        assert name in capi.SYMBOLS
    assert hasattr(capi.Bank, "set_window") and hasattr(capi.Group, "set_window")


@pytest.mark.parametrize("n", [512, 4096, 65536])
def test_hann_is_its_formula(n):
    w = synth.hann(n)
    assert w.dtype == np.float32 and w.shape == (n,)
    assert w[0] == 0.0 and w[n // 2] == 1.0
    want = np.array([np.float32(0.5 - 0.5 * np.cos(2.0 * np.pi * i / n)) for i in range(n)], np.float32)
    assert np.array_equal(w.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(w[1:], w[:0:-1])  # periodic: symmetric about n / 2, w[n - i] == w[i]
    assert abs(float(w.astype(np.float64).mean()) - 0.5) < 1e-6  # coherent gain 0.5 = -6.02 dB
    assert abs(float((w.astype(np.float64) ** 2).mean()) - 0.375) < 1e-6  # power gain 0.375 = -4.26 dB


def test_windowed_frames_are_one_float32_product():
    """The oracle side of every comparison: each component times its sample's window value, rounded once to float32."""
    rng = np.random.default_rng(3)
    n = 512
    f = rng.standard_normal((3, 2 * n)).astype(np.float32)
    w = rng.random(n, dtype=np.float32)
    got = windowed(f, w, n)
    want = (f.astype(np.float64).reshape(3, n, 2) * w.astype(np.float64)[None, :, None]).astype(np.float32).reshape(3, 2 * n)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))  # (24 x 24 bits fit a double)
    assert np.array_equal(windowed(f, np.ones(n, np.float32), n).view(np.uint32), f.view(np.uint32))


def test_batch_plan_never_puts_a_windowed_bank_on_r32(tmp_path):
    exe = str(tmp_path / "test_batch_plan_window")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                         os.path.join(HOST, "test_batch_plan_window.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.split() == ["plan", "ok"]


@pytest.mark.parametrize("neighbour", ["carrier", "soft"])
def test_the_oracle_needs_the_window(neighbour):
    """Measured with the oracle over the stream's 72 cumulations - rectangular / Hann: 'dl1abc' read 0 / 6 times (unkeyed
    neighbour) and 0 / 5 times (soft-keyed, its message repeated behind a word gap for the whole stream); the two stations
    one peak run in 72 / 0 and 63 / 0 cumulations; longest run 346 / 12 and 231 / 12 bins."""
    s = demo_stream(neighbour)
    rect, hann = demo_oracle(s, None), demo_oracle(s, synth.hann(DEMO["n"]))
    print(neighbour, "rectangular:", repr(rect["text"]), merged_runs(rect["peaks"]), "hann:", repr(hann["text"]), merged_runs(hann["peaks"]),
          "cumulations", len(rect["peaks"]))
    check_demo_oracle(rect, hann)
