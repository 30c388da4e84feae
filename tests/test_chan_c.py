"""The channelizer from PLAIN C (tests/host/test_chan_c.c).

CPU: the program compiles as C11 under -Wall -Werror -pedantic against include/sdrainer_hip.h (it takes every sdr_chan_*
entry point by address, with its declared type) and links against the library and the HIP runtime.
GPU: its argument checks return their statuses, and a stream processed from C in two sdr_chan_process_host calls gives the
bits of tests/chan_ref.py for every output of every selected channel."""
import os
import re
import subprocess

import numpy as np
import pytest

import chan_ref as CR
import ddc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_chan_c.c")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sdrainer_amd.csrc import build
    lib = build.build()
    out = str(tmp_path_factory.mktemp("chan_c") / "test_chan_c")
    libdir = os.path.dirname(lib)
    hipdir = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "lib")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-O1", "-o", out, SRC, "-L" + libdir,
                           "-l:" + os.path.basename(lib), "-Wl,-rpath," + libdir, "-L" + hipdir, "-lamdhip64", "-Wl,-rpath," + hipdir])
    return out


def test_chan_entry_points_are_plain_c(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr


def test_every_chan_declaration_is_taken():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrainer_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(sdr_chan_\w+)\s*\(", header)))
    assert len(declared) == 9, declared
    src = open(SRC).read()
    for name in declared:
        assert re.search(r"= " + name + ";", src), name


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [R.CU8, CR.RR.RS16], ids=["cu8", "rs16"])
def test_plain_c_chan_stream(exe, tmp_path, fmt):
    from sdrainer_amd import capi

    m, d, p, channels = 16, 8, 3, (15, 0, 5, 8)
    taps = np.random.default_rng(21).uniform(-1, 1, m * p).astype(np.float32)
    raw = CR.random_raw(d * 90, fmt, 22 + fmt)
    raw.tofile(str(tmp_path / "raw.bin"))
    taps.tofile(str(tmp_path / "taps.f32"))
    p = subprocess.run([exe, str(tmp_path / "raw.bin"), str(fmt), str(m), str(d), str(tmp_path / "taps.f32"), str(len(taps)), str(len(raw))]
                       + [str(c) for c in channels], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert lines[0] == "outputs 90" and lines[-1] == "done" and len(lines) == 2 + len(channels)
    want = CR.chan_ref(CR.to_f32(raw, fmt), m, d, taps, *capi.ddc_nco_table(), channels=channels)
    for b in range(len(channels)):
        got = np.array([int(w, 16) for w in lines[1 + b].split()[1:]], np.uint32)
        assert np.array_equal(got, want[b].reshape(-1).view(np.uint32)), f"stream {b}"
