"""The receive chain from PLAIN C (tests/host/test_chain_c.c), without a GPU: the program compiles as C11 under -Wall -Werror
-pedantic against include/sdrainer_hip.h, takes the ten entry points by address with their declared types, links against the
library and runs: the size and every field offset of sdr_chain_config and sdr_chain_counts are the ctypes structures', the ABI
version stays 2, null handles and configurations without members are refused, and the values of sdr_chain_granule and
sdr_chain_min_ring are tests/chain_ref.py's."""
import ctypes
import os
import re
import subprocess

import pytest

import chain_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_chain_c.c")
NAMES = ["sdr_chain_create", "sdr_chain_destroy", "sdr_chain_set_stream", "sdr_chain_sync", "sdr_chain_push_host",
         "sdr_chain_push_device", "sdr_chain_read_narrow", "sdr_chain_stats", "sdr_chain_granule", "sdr_chain_min_ring"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sdrainer_amd.csrc import build
    lib = build.build()
    out = str(tmp_path_factory.mktemp("chain_c") / "test_chain_c")
    libdir = os.path.dirname(lib)
    hipdir = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "lib")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-O1", "-o", out, SRC, "-L" + libdir,
                           "-l:" + os.path.basename(lib), "-Wl,-rpath," + libdir, "-L" + hipdir, "-lamdhip64", "-Wl,-rpath," + hipdir])
    return out


def test_layout_refusals_and_the_host_calls_from_plain_c(exe):
    from sdrainer_amd import capi

    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    lines = [ln.split() for ln in p.stdout.splitlines()]
    assert p.returncode == 0 and lines[-1] == ["layout", "ok"], p.stdout + p.stderr
    structs = {"sdr_chain_config": capi.ChainConfig, "sdr_chain_counts": capi.ChainCounts}
    sizes = {w[1]: int(w[2]) for w in lines if w[0] == "size"}
    assert sizes == {name: ctypes.sizeof(s) for name, s in structs.items()} and sizes["sdr_chain_config"] == 56
    for name, s in structs.items():
        got = [(w[2], int(w[3])) for w in lines if w[0] == "field" and w[1] == name]
        assert got == [(f, getattr(s, f).offset) for f, _ in s._fields_], name
    granules = [[int(v) for v in w[1:]] for w in lines if w[0] == "granule"]
    rings = [[int(v) for v in w[1:]] for w in lines if w[0] == "min_ring"]
    assert len(granules) == 11 and len(rings) == 12
    for dtot, nb, value in granules:
        assert value == CR.granule(dtot, nb), (dtot, nb)
    for block, hop, piece, dtot, value in rings:
        assert value == CR.min_ring(block, hop, piece, dtot), (block, hop, piece, dtot)
    assert sum(g[2] < 0 for g in granules) == 4 and sum(r[4] < 0 for r in rings) == 8


def test_every_chain_declaration_is_taken():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sdrainer_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(sdr_chain_\w+)\s*\(", header)))
    assert declared == sorted(NAMES)
    src = open(SRC).read()
    for name in declared:
        assert re.search(r"= " + name + ";", src), name
    from sdrainer_amd import capi
    assert all(n in capi.SYMBOLS for n in NAMES)
    # the sets of the other front-end calls and the ABI version stay what they were
    for prefix, count in (("sdr_ddc_", 10), ("sdr_chan_", 9), ("sdr_iq_", 7), ("sdr_nb_", 12), ("sdr_fine_", 10)):
        assert len(set(re.findall(r"\b(" + prefix + r"\w+)\s*\(", header))) == count, prefix
    assert re.search(r"#define SDR_ABI_VERSION 2\b", header)
