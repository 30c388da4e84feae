"""The IQ correction from PLAIN C (tests/host/test_iqc_c.c), without a GPU: the program compiles as C11 under -Wall -Werror
-pedantic against include/sdrainer_hip.h - sizeof(sdr_iq_correction) == 16, sizeof(sdr_iq_sums) == 64 and every field offset
are static assertions in it, and it takes the seven new entry points by address with their declared types - links against
the library, and runs: null handles are refused, sdr_iq_correction_from_sums refuses n = 1 without touching its output and
undoes an exactly representable imbalance."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_iqc_c.c")
NAMES = ["sdr_iq_ddc_set_correction", "sdr_iq_ddc_enable_sums", "sdr_iq_ddc_read_sums", "sdr_iq_chan_set_correction",
         "sdr_iq_chan_enable_sums", "sdr_iq_chan_read_sums", "sdr_iq_correction_from_sums"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sdrainer_amd.csrc import build
    lib = build.build()
    out = str(tmp_path_factory.mktemp("iqc_c") / "test_iqc_c")
    libdir = os.path.dirname(lib)
    hipdir = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "lib")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-O1", "-o", out, SRC, "-L" + libdir,
                           "-l:" + os.path.basename(lib), "-Wl,-rpath," + libdir, "-L" + hipdir, "-lamdhip64", "-Wl,-rpath," + hipdir])
    return out


def test_layout_and_host_entry_point_from_plain_c(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.split() == ["layout", "ok"], p.stdout + p.stderr


def test_every_iq_declaration_is_taken():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrainer_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(sdr_iq_\w+)\s*\(", header)))
    assert declared == sorted(NAMES)
    src = open(SRC).read()
    for name in declared:
        assert re.search(r"= " + name + ";", src), name
    from sdrainer_amd import capi
    assert all(n in capi.SYMBOLS for n in NAMES)
    import ctypes
    assert ctypes.sizeof(capi.IqCorrection) == 16 and ctypes.sizeof(capi.IqSums) == 64
    assert ctypes.sizeof(capi.DdcConfig) == 32 and ctypes.sizeof(capi.ChanConfig) == 32
