"""The host mirror's listener reports (sdrainer_amd/csrc/host/rx.h: Receiver::EnableReports / ListenerLevel), driven by
tests/host/test_rx_reports.cpp: a decode-mode receiver on one keyed carrier.  The listener's totals after the whole stream -
every polled segment's record added up - equal the numpy totals (tests/reports_ref.py) over the oracle's whole-stream trace,
integers and the bits of wpm, whatever the segments' length."""
import json
import os
import subprocess

import numpy as np
import pytest

import reports_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdrainer_amd", "csrc")
RATE, N, FRAMES, TONES, SEED, CENTER = 48000, 512, 1400, 3, 9, 7020000


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    from sdrainer_amd.csrc import build
    build.build()
    out = str(tmp_path_factory.mktemp("rx_reports") / "test_rx_reports")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", "-o", out, os.path.join(ROOT, "tests", "host", "test_rx_reports.cpp"),
                           "-L" + CSRC, "-lsdrainer_hip", "-Wl,-rpath," + CSRC])
    return out


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    """The input file, the listened bin and the oracle's totals for it over the whole stream."""
    from oracle import oracle as orc
    from sdrainer_amd import synth

    iq, bins, _ = synth.make_band(FRAMES, RATE, N, TONES, seed=SEED)
    sb = int(bins[1])
    path = tmp_path_factory.mktemp("rx_reports_in") / "iq.f32"
    iq.astype(np.float32).tofile(path)
    r = orc.Receiver(RATE, N, 70, 15.0, 1, center_frequency=CENTER)
    lid = r.attach(sb)
    out = r.process(iq)
    want = ref.report(out["values"][:, lid], out["deb"][:, lid], out["frames"]["noise_floor"])
    want.update(band=0, listener=0, bin=sb, wpm=float(r.decoder_state(lid)[3]))
    assert want["ticks_on"] >= 300 and want["ticks_off"] >= 300, want  # a keyed carrier: both levels are measured
    return str(path), sb, want


def test_program_builds_and_says_how_it_is_called(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("max_batch", [64, 256])
def test_listener_level_totals(exe, stream, max_batch):
    path, sb, want = stream
    offset = int((sb - N // 2) * RATE / N) + 20  # a frequency inside bin sb, relative to the centre
    p = subprocess.run([exe, path, str(RATE), str(N), str(FRAMES), str(offset), str(max_batch)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = json.loads(p.stdout)
    assert got["frames"] == FRAMES and got["id"] == "rx1" and got["events"] == 1
    got["wpm"] = float(np.uint64(got["wpm_bits"]).view(np.float64))
    bad = ref.same(got, want)
    assert not bad, f"fields {bad}: {got} != {want}"
