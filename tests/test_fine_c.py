"""The fine converter from PLAIN C (tests/host/test_fine_c.c), without a GPU: the program compiles as C11 under -Wall -Werror
-pedantic against include/sdrainer_hip.h - sizeof(sdr_fine_config) == 32 and every field offset are static assertions in it,
and it takes the ten entry points by address with their declared types - links against the library, and runs: null handles
and bad configurations are refused, and the values sdr_fine_tune prints are the integer definition's (tests/fine_ref.py
tune_ref)."""
import os
import re
import subprocess

import pytest

import fine_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_fine_c.c")
NAMES = ["sdr_fine_create", "sdr_fine_destroy", "sdr_fine_sync", "sdr_fine_set_stream", "sdr_fine_set_first_sample",
         "sdr_fine_total_samples", "sdr_fine_set_nco_step", "sdr_fine_set_input", "sdr_fine_process_device", "sdr_fine_tune"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sdrainer_amd.csrc import build
    lib = build.build()
    out = str(tmp_path_factory.mktemp("fine_c") / "test_fine_c")
    libdir = os.path.dirname(lib)
    hipdir = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "lib")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-O1", "-o", out, SRC, "-L" + libdir,
                           "-l:" + os.path.basename(lib), "-Wl,-rpath," + libdir, "-L" + hipdir, "-lamdhip64", "-Wl,-rpath," + hipdir])
    return out


def test_layout_refusals_and_tuning_from_plain_c(exe):
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    lines = p.stdout.splitlines()
    assert p.returncode == 0 and lines[-1].split() == ["layout", "ok"], p.stdout + p.stderr
    tunes = [[int(v) for v in ln.split()[1:]] for ln in lines if ln.startswith("tune ")]
    assert len(tunes) == 13 and len(tunes) == len(lines) - 1
    refused = 0
    for m, d, target, rc, ch, st in tunes:
        legal = m in (2, 4, 8, 16, 32, 64, 128, 256) and d >= 1 and d in (m, m // 2, m // 4) and abs(target) <= 32768 * d
        if legal:
            assert rc == 0 and (ch, st) == F.tune_ref(m, d, target), (m, d, target)
        else:
            assert rc == 1 and (ch, st) == (-7, -9), (m, d, target)  # SDR_ERR_BAD_ARG, the outputs untouched
            refused += 1
    assert refused == 4 and tunes[0][3:] == [0, 1, 4800] and tunes[1][3:] == [0, 6, -6400]


def test_every_fine_declaration_is_taken():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrainer_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(sdr_fine_\w+)\s*\(", header)))
    assert declared == sorted(NAMES)
    src = open(SRC).read()
    for name in declared:
        assert re.search(r"= " + name + ";", src), name
    from sdrainer_amd import capi
    assert all(n in capi.SYMBOLS for n in NAMES)
    import ctypes
    assert ctypes.sizeof(capi.FineConfig) == 32
    # the sets of the other front-end calls stay what they were
    for prefix, count in (("sdr_ddc_", 10), ("sdr_chan_", 9), ("sdr_iq_", 7), ("sdr_nb_", 12)):
        assert len(set(re.findall(r"\b(" + prefix + r"\w+)\s*\(", header))) == count, prefix
