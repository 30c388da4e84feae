"""The group entry points from PLAIN C (tests/host/test_group_c.c): the C half of a cgo shim that drives several GPUs
from one process.

CPU: the program compiles as C11 under -Wall -Werror -pedantic against include/sdrainer_hip.h and links against the
library.
GPU: it drives a two-member group (both members on device 0) of three bands: create -> push_iq -> process_staged ->
attach through sdr_group_member -> push / process -> poll -> destroy.  The keying edges and the decoded text it prints
for every band equal the oracle's run of that band (listeners attached behind the first cumulation, as
rx/receiver.go:409-426 binds them), with the bands numbered as one bank numbers them."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_group_c.c")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sdrainer_amd.csrc import build
    lib = build.build()
    out = str(tmp_path_factory.mktemp("group_c") / "test_group_c")
    libdir = os.path.dirname(lib)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-O1", "-o", out, SRC, "-L" + libdir,
                           "-l:" + os.path.basename(lib), "-Wl,-rpath," + libdir])
    return out


def test_group_entry_points_are_plain_c(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr


@pytest.mark.gpu
def test_plain_c_group_end_to_end(exe, tmp_path):
    from oracle import oracle as orc
    from sdrainer_amd import synth

    n, rate, tones, frames, bands = 1024, 96000, 4, 600, 3
    edge = synth.default_edge_width(n)
    made = [synth.make_band(frames, rate, n, tones, seed=6100 + b) for b in range(bands)]
    bins = made[0][1]  # (tone_bins depends on the geometry only: the same bins on every band)
    assert all(np.array_equal(m[1], bins) for m in made)
    path = str(tmp_path / "iq.f32")
    np.ascontiguousarray(np.stack([m[0] for m in made]), dtype=np.float32).tofile(path)
    p = subprocess.run([exe, path, str(rate), str(n), str(frames), str(edge), str(bands), "2", "0", "0", "--"] +
                       [str(int(b)) for b in bins], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert lines[-1] == "done" and "total dropped 0 0" in lines
    assert [ln for ln in lines if ln.startswith("batch")] == ["batch 0 first_frame 0 frames 100", f"batch 1 first_frame 100 frames {frames - 100}"]
    assert [ln for ln in lines if ln.startswith("attached")] == [
        f"attached band {b} bin {int(t)} -> member {b % 2} local {b // 2} id {i}" for b in range(bands) for i, t in enumerate(bins)]
    # chunks: band by band, each band's cumulations in order
    assert [ln.split()[2] for ln in lines if ln.startswith("chunk")] == ["0", "1", "2"] + ["0"] * 5 + ["1"] * 5 + ["2"] * 5
    total_runes = 0
    for b in range(bands):
        iq = made[b][0]
        ref = orc.Receiver(rate, n, edge, 15.0, 1)
        ref.process(iq[:100])
        for t in bins:
            ref.attach(int(t))
        out = ref.process(iq[100:])
        deb = out["deb"].astype(np.int8)
        for lid in range(tones):
            trans = np.flatnonzero(np.diff(np.concatenate([[0], deb[:, lid]])) != 0)
            edges = " ".join(f"{int(t) + 100}:{int(deb[t, lid])}" for t in trans)
            got = [ln for ln in lines if ln.startswith(f"listener {b} {lid} edges")]
            assert got == [f"listener {b} {lid} edges" + (" " + edges if edges else "")], (b, lid)
            runes = [ln for ln in lines if ln.startswith(f"listener {b} {lid} runes")][0].split()[4:]
            assert "".join(chr(int(r)) for r in runes) == ref.text(lid), (b, lid)
            total_runes += len(runes)
    assert total_runes > 0
