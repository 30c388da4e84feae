"""The 8-bit entry points from PLAIN C (tests/host/test_iq8_c.c).

CPU: the program compiles as C11 under -Wall -Werror -pedantic against include/sdrainer_hip.h (it takes every 8-bit entry
point by address, with its declared type), links against the library, and names every *_iq8 declaration of the header.
GPU: the program's argument checks return their statuses (formats 2 and -1, null pointers, rate, size, nothing captured),
and a short batch pushed from C (sdr_push_iq8 -> sdr_process_staged) gives the oracle's psd of the converted values for its
last frame, bit for bit, in both formats."""
import os
import re
import subprocess

import numpy as np
import pytest

import iq8_tools as t8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_iq8_c.c")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sdrainer_amd.csrc import build
    lib = build.build()
    out = str(tmp_path_factory.mktemp("iq8_c") / "test_iq8_c")
    libdir = os.path.dirname(lib)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-O1", "-o", out, SRC, "-L" + libdir,
                           "-l:" + os.path.basename(lib), "-Wl,-rpath," + libdir])
    return out


def test_iq8_entry_points_are_plain_c(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr


def test_every_iq8_declaration_is_taken():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrainer_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(sdr_\w*iq8)\s*\(", header)))
    assert len(declared) == 7, declared
    src = open(SRC).read()
    for name in declared:
        assert re.search(r"= " + name + ";", src), name
    assert re.search(r"#define SDR_IQ8_CS8 0\b", header) and re.search(r"#define SDR_IQ8_CU8 1\b", header)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", t8.FORMATS, ids=t8.FORMAT_IDS)
def test_plain_c_iq8_batch(exe, tmp_path, fmt):
    from oracle import oracle as orc

    n, frames = 1024, 21
    q, _, _ = t8.pool(n, 4, 6300 + fmt, fmt, frames=frames, oracle_psd=False)
    path = str(tmp_path / "iq.u8")
    q.tofile(path)
    p = subprocess.run([exe, path, str(t8.RATE[n]), str(n), str(frames), str(fmt)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert lines[0] == f"frames {frames}" and lines[-1] == "done"
    got = np.array([int(w, 16) for w in lines[1].split()[1:]], np.uint32)
    want = orc.iq_to_spectrum_and_psd(t8.to_f32(q[-1], fmt))[1].view(np.uint32)
    assert np.array_equal(got, want)
