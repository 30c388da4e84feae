"""The sc16 entry points from PLAIN C (tests/host/test_sc16_c.c).

CPU: the program compiles as C11 under -Wall -Werror -pedantic against include/sdrainer_hip.h (it takes every sc16 entry
point by address, with its declared type) and links against the library.
GPU: a short sc16 batch pushed from C (sdr_push_iq_sc16 -> sdr_process_staged) gives the oracle's psd of
float32(x) / 32767 for its last frame, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_sc16_c.c")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sdrainer_amd.csrc import build
    lib = build.build()
    out = str(tmp_path_factory.mktemp("sc16_c") / "test_sc16_c")
    libdir = os.path.dirname(lib)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-O1", "-o", out, SRC, "-L" + libdir,
                           "-l:" + os.path.basename(lib), "-Wl,-rpath," + libdir])
    return out


def test_sc16_entry_points_are_plain_c(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr


@pytest.mark.gpu
def test_plain_c_sc16_batch(exe, tmp_path):
    from oracle import oracle as orc
    from sdrainer_amd import synth

    n, rate, frames = 1024, 96000, 21
    iq, _, _ = synth.make_band(frames, rate, n, 4, seed=6200)
    q = np.clip(np.rint(iq.astype(np.float64) * 3.0e5), -32768, 32767).astype("<i2")
    path = str(tmp_path / "iq.s16")
    q.tofile(path)
    p = subprocess.run([exe, path, str(rate), str(n), str(frames)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert lines[0] == f"frames {frames}" and lines[-1] == "done"
    got = np.array([int(w, 16) for w in lines[1].split()[1:]], np.uint32)
    want = orc.iq_to_spectrum_and_psd(q[-1].astype(np.float32) / np.float32(32767))[1].view(np.uint32)
    assert np.array_equal(got, want)
