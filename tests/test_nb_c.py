"""The impulse noise blanker from PLAIN C (tests/host/test_nb_c.c), without a GPU: the program compiles as C11 under -Wall
-Werror -pedantic against include/sdrainer_hip.h - sizeof(sdr_nb_config) == 32, sizeof(sdr_nb_stats) == 32 and every field
offset are static assertions in it, and it takes the twelve entry points by address with their declared types - links against
the library, and runs: null handles are refused, and sdr_nb_blank_host blanks one planted impulse of a 128-sample cs8
stream and its hold."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_nb_c.c")
NAMES = ["sdr_nb_create", "sdr_nb_destroy", "sdr_nb_sync", "sdr_nb_set_stream", "sdr_nb_set_first_sample", "sdr_nb_total_samples",
         "sdr_nb_set_threshold", "sdr_nb_process_device", "sdr_nb_process_host", "sdr_nb_read_stats", "sdr_nb_tile_samples",
         "sdr_nb_blank_host"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sdrainer_amd.csrc import build
    lib = build.build()
    out = str(tmp_path_factory.mktemp("nb_c") / "test_nb_c")
    libdir = os.path.dirname(lib)
    hipdir = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "lib")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-O1", "-o", out, SRC, "-L" + libdir,
                           "-l:" + os.path.basename(lib), "-Wl,-rpath," + libdir, "-L" + hipdir, "-lamdhip64", "-Wl,-rpath," + hipdir])
    return out


def test_layout_and_host_entry_points_from_plain_c(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.split() == ["layout", "ok"], p.stdout + p.stderr


def test_every_nb_declaration_is_taken():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrainer_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(sdr_nb_\w+)\s*\(", header)))
    assert declared == sorted(NAMES)
    src = open(SRC).read()
    for name in declared:
        assert re.search(r"= " + name + ";", src), name
    from sdrainer_amd import capi
    assert all(n in capi.SYMBOLS for n in NAMES)
    import ctypes
    assert ctypes.sizeof(capi.NbConfig) == 32 and ctypes.sizeof(capi.NbStats) == 32
    # the sets of the other front-end calls stay what they were
    for prefix, count in (("sdr_ddc_", 10), ("sdr_chan_", 9), ("sdr_iq_", 7)):
        assert len(set(re.findall(r"\b(" + prefix + r"\w+)\s*\(", header))) == count, prefix
