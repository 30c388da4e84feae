"""What the default seeds of tests/test_gpu_fuzz_paths.py reach, without a GPU: the batch plan (host/batch_plan.h, driven
by tests/host/fuzz_paths_plan.cpp) of every batch they make, their input paths, listener events and adversarial kinds.
A later edit that shrinks the generator's reach fails here.  And the tied-window frames are refused by noise_cert.h's
certify() itself (tests/host/cert_rows.cpp), so that they keep testing the literal loops' first-minimum rule."""
import os
import subprocess

import numpy as np
import pytest

import fuzz_paths_gen as gen
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")


def _compile(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    cc = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra, "-o", exe, os.path.join(HOST, name + ".cpp")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    return exe


def _batches(s):
    """(plan input line, seed, batch index) of every batch of seed s, as the bank would plan it."""
    steps, init = s.steps([[100 + i for i in range(b["tones"])] for b in s.bands])  # (bins do not change the plan)
    slots = [len(x) for x in init]  # the slot pool is a high-water mark: a detach leaves it as it is
    graph = s.path.startswith("graph")
    max_frames = max(st[1] for st in steps if st[0] in ("batch", "defer"))
    pos, out = 0, []
    for st in steps:
        if st[0] == "attach":
            slots[st[1]] += 1
        elif st[0] in ("batch", "defer"):
            out.append(f"{s.n} {s.n_bands} {max_frames} {st[1]} {pos % 100} {int(graph)} {max(slots)}")
            for band, _, _ in st[2] if st[0] == "defer" else []:
                slots[band] += 1  # (sdr_attach_at after the batch's FFT: the next batch's)
            pos += st[1]
    return steps, out


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = _compile(tmp_path_factory.mktemp("plan"), "fuzz_paths_plan")
    seeds = [gen.Seed(i) for i in range(gen.DEFAULT_SEEDS)]
    lines, rows = [], []
    for s in seeds:
        steps, ls = _batches(s)
        lines += ls
        rows += [(s, steps)] * len(ls)
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    plan = [tuple(int(x) for x in ln.split()) for ln in run.stdout.split("\n") if ln]
    assert len(plan) == len(lines)
    return seeds, [(s, steps, dict(zip(("r32", "wide_tap", "two_phase", "group_frames", "scan_parts", "gather_peaks", "noise_scan", "bound"), p)),
                    int(line.split()[3]))
                   for (s, steps), p, line in zip(rows, plan, lines)]


def test_default_seeds_reach_every_size_path_and_kind(plans):
    seeds, _ = plans
    for n in gen.SIZES:
        assert any(s.n == n and s.path not in gen.SC16_PATHS for s in seeds), f"N = {n}: no float32 seed"
        assert any(s.n == n and s.path in gen.SC16_PATHS for s in seeds), f"N = {n}: no sc16 seed"
    for path in ("staged", "staged_sc16", "kiwi"):
        assert any(s.path == path and s.n <= 16384 for s in seeds) and any(s.path == path and s.n > 16384 for s in seeds), path
    assert set(gen.PATHS) <= {s.path for s in seeds}
    assert set(gen.KINDS) <= {s.kind for s in seeds}
    for fam in ("psd", "16384", "2p"):
        assert any(gen.family(s.n) == fam and s.n_bands >= 2 for s in seeds), f"{fam}: no seed of two bands or more"


def test_default_seeds_reach_every_plan(plans):
    _, rows = plans
    assert any(p["r32"] and p["wide_tap"] for _, _, p, _ in rows), "k_fft_r32 with its wide tap"
    assert any(p["r32"] and not p["wide_tap"] for _, _, p, _ in rows), "k_fft_r32 without listeners (no wide tap)"
    assert any(s.n == 16384 and not p["r32"] and f * s.n_bands < 1024 for s, _, p, f in rows), "k_fft_psd<14>: a short launch"
    assert any(s.n == 16384 and not p["r32"] and f * s.n_bands >= 1024 for s, _, p, f in rows), "k_fft_psd<14>: more than 512 slots"
    for n in (32768, 65536):
        assert any(s.n == n and p["two_phase"] and f > p["group_frames"] for s, _, p, f in rows), f"two-phase at {n} across frame groups"
    assert {p["scan_parts"] for _, _, p, _ in rows} >= {1, 2}
    assert {p["gather_peaks"] for _, _, p, _ in rows} == {0, 1}, "the gather on the peaks stream and on the listen stream"
    assert any(f == 1 for _, _, _, f in rows), "one-frame batches"
    assert any((sum(x[1] for x in steps[:i] if x[0] in ("batch", "defer")) % 100) + x[1] > 100
               for s, steps, _, _ in rows for i, x in enumerate(steps) if x[0] == "batch"), "batches across cumulation boundaries"


def test_default_seeds_reach_every_listener_event(plans):
    seeds, rows = plans
    kinds = set()
    for s, steps, _, _ in rows:
        for i, st in enumerate(steps):
            if st[0] in ("attach", "detach"):
                kinds.add(st[0])
                if s.path.startswith("graph") and i > 0 and any(x[0] == "batch" for x in steps[i:]):
                    kinds.add("recapture")
            if st[0] == "defer" and st[2]:
                kinds.add("attach_at")
    assert kinds == {"attach", "detach", "attach_at", "recapture"}


def _cert_rows(tmp_path, exe, rows, n, edge):
    f = tmp_path / "rows.f32"
    np.ascontiguousarray(rows, np.float32).tofile(str(f))
    run = subprocess.run([exe, str(f), str(n), str(edge)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    return [tuple(int(x) for x in ln.split()) for ln in run.stdout.split("\n") if ln]


def test_tied_window_frames_are_refused_by_the_certificate(tmp_path):
    """certify() on the oracle's psd rows of tied-window frames (the window sums formed in the reference's order, so that
    they are exactly equal): not accepted - its minimum's bracket overlaps every other window's (why 2) - and the literal
    loops take window 0.  Ordinary frames of the same seeds are accepted."""
    exe = _compile(tmp_path, "cert_rows", ["-ffp-contract=off"])
    seeds = [gen.Seed(i) for i in range(gen.DEFAULT_SEEDS)]
    seeds = [s for s in seeds if s.kind == "tied_windows"]
    seeds += [gen.Seed(5000 + gen.SIZES.index(n), n=n, path="staged", kind="tied_windows") for n in gen.SIZES]
    assert {s.n for s in seeds} == set(gen.SIZES)
    for s in seeds:
        bands = s.inputs()
        iq = bands[s.adv_band][0]
        tied = s.tied_frames[:4]
        ordinary = [f for f in range(s.total) if f not in set(s.tied_frames)][:4]
        rows = [orc.iq_to_spectrum_and_psd(iq[f])[1] for f in list(tied) + ordinary]
        got = _cert_rows(tmp_path, exe, rows, s.n, s.edge)
        assert got[:len(tied)] == [(0, 2, 0)] * len(tied), (s.seed, s.n, got)
        assert sum(ok for ok, _, _ in got[len(tied):]) >= len(ordinary) - 1, (s.seed, s.n, got)


def test_forced_selection_covers_families_paths_and_kinds():
    sel = [gen.Seed(i) for i in gen.forced_selection()]
    assert {gen.family(s.n) for s in sel} == {"psd", "16384", "2p"}
    assert {s.path for s in sel} == set(gen.PATHS)
    assert {s.kind for s in sel} >= set(gen.KINDS[1:])
