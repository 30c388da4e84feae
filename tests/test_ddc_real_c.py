"""The down-converter's real input from PLAIN C (tests/host/test_ddc_real_c.c), in the manner of tests/test_ddc_c.py.

CPU: the program compiles as C11 under -Wall -Werror -pedantic against include/sdrainer_hip.h - the real formats are
constant expressions of the header, sdr_ddc_config is 32 bytes - and links against the library and the HIP runtime.
GPU: an int16 real stream processed from C in two sdr_ddc_process_host calls of an SDR_DDC_RS16 DDC gives the bits of
tests/ddc_ref.py fed (value, +0.0) for every output of every band."""
import os
import subprocess

import numpy as np
import pytest

import ddc_real as DR
import ddc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_ddc_real_c.c")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sdrainer_amd.csrc import build
    lib = build.build()
    out = str(tmp_path_factory.mktemp("ddc_real_c") / "test_ddc_real_c")
    libdir = os.path.dirname(lib)
    hipdir = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "lib")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-O1", "-o", out, SRC, "-L" + libdir,
                           "-l:" + os.path.basename(lib), "-Wl,-rpath," + libdir, "-L" + hipdir, "-lamdhip64", "-Wl,-rpath," + hipdir])
    return out


def test_real_ddc_caller_is_plain_c(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr


@pytest.mark.gpu
def test_plain_c_real_ddc_stream(exe, tmp_path):
    from sdrainer_amd import capi

    d, t, steps = 6, 48, (9000, -32768, -9000)
    taps = np.random.default_rng(21).uniform(-1, 1, t).astype(np.float32)
    raw = DR.random_raw_real(d * 90, DR.RS16, 23)
    assert raw.dtype == np.int16 and raw.ndim == 1
    raw.tofile(str(tmp_path / "raw.bin"))
    taps.tofile(str(tmp_path / "taps.f32"))
    p = subprocess.run([exe, str(tmp_path / "raw.bin"), str(d), str(tmp_path / "taps.f32"), str(t), str(len(raw))] + [str(s) for s in steps],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert lines[0] == "outputs 90" and lines[-1] == "done" and len(lines) == 2 + len(steps)
    want = R.ddc_ref(DR.as_complex(DR.to_f32_real(raw, DR.RS16)), d, taps, steps, *capi.ddc_nco_table())
    for b in range(len(steps)):
        got = np.array([int(w, 16) for w in lines[1 + b].split()[1:]], np.uint32)
        assert np.array_equal(got, want[b].reshape(-1).view(np.uint32)), f"band {b}"
