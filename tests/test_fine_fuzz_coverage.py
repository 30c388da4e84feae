"""What the default seeds of tests/test_fine_fuzz_gpu.py reach, proved without a GPU: tests/host/ddc_shape_probe.cpp (the
probe of tests/test_ddc_fuzz_coverage.py) prints sdr::ddc_shape of the library's own header, which launch_fine calls, so the
shape of every seed is the launcher's; the seeds reach every one of the nine tile shapes twice, with both example geometries
where the table has two, every value kind, event and first-sample kind, every input count up to 256, a map with shared
inputs and an unread one, input and output gaps of 0 and more; and the reference alone, run over every seed, agrees with
fine_ref.FineRef run call by call - with the events and without - and holds each value kind's condition."""
import os
import subprocess

import numpy as np
import pytest

import ddc_fuzz_gen as dgen
import fine_fuzz_gen as gen
from parity_tools import bits_equal, capi, nan_equal_bits  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ddc_shape_probe.cpp")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """ask(pairs) -> {(D, T): (chunk, threads, width, lds_bytes)} from the library's header."""
    from sdrainer_amd.csrc import build as hip_build

    cc = hip_build.hipcc()
    roots = [os.path.dirname(os.path.dirname(p)) for p in (cc, os.path.realpath(cc))] + [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    include = next(os.path.join(r, "include") for r in roots if r and os.path.isfile(os.path.join(r, "include", "hip", "hip_runtime.h")))
    exe = str(tmp_path_factory.mktemp("fine_shape") / "ddc_shape_probe")
    done = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + include, "-o", exe, SRC],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr

    def ask(pairs):
        run = subprocess.run([exe] + [str(v) for p in pairs for v in p], capture_output=True, text=True, timeout=300)
        assert run.returncode == 0 and not run.stderr, run.stdout[-2000:] + run.stderr[-2000:]
        rows = [[int(w) for w in line.split()] for line in run.stdout.splitlines()]
        return {(r[0], r[1]): tuple(r[2:]) for r in rows}
    return ask


@pytest.fixture(scope="module")
def seeds():
    return gen.seeds()


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


def test_the_tables_are_the_down_converter_fuzzes():
    for name in ("TABLE", "CLASSES", "shape", "TILE", "PLANTS", "BANDS", "FIRSTS", "COST_CAP"):
        assert getattr(gen, name) is getattr(dgen, name), name


def test_default_seeds_reach_every_shape_twice(probe, seeds):
    assert len(seeds) == gen.DEFAULT_SEEDS == 18 and len(gen.CLASSES) == 9
    shapes = probe(sorted({(s.d, s.t) for s in seeds}))
    for s in seeds:
        assert shapes[(s.d, s.t)] == (s.chunk, s.threads, s.width, s.lds_bytes) == gen.shape(s.d, s.t), s.ident
        assert s.cls == (s.chunk, s.threads)
    assert [s.cls for s in seeds] == list(gen.CLASSES) * 2
    for cls, examples in gen.TABLE:
        assert {(s.d, s.t) for s in seeds if s.cls == cls} == {examples[0], examples[-1]}, cls
        assert len(examples) == 1 or examples[0] != examples[-1]
    # the shapes tests/test_fine_gpu.py does not reach: a second output in some lanes only, narrower workgroups, the odd chunk
    assert {(448, 256), (384, 256), (320, 256), (192, 192), (128, 128), (63, 64)} <= {s.cls for s in seeds}
    assert {s.threads % s.d for s in seeds if s.threads < 256} >= {192 % 100, 128 % 150, 64 % 255}
    assert any(s.t == 1 for s in seeds) and any(s.t == 4096 for s in seeds)  # no carry at all, and the longest
    assert max(s.lds_bytes for s in seeds) >= 163_000 and all(s.lds_bytes <= dgen.MAX_LDS for s in seeds)
    assert len({s.ident for s in seeds}) == len(seeds)


def test_default_seeds_reach_every_kind_map_and_event(seeds):
    assert {s.kind for s in seeds} == set(gen.KINDS)
    assert all(s.chunk <= s.threads for s in seeds if s.kind == "zeros")  # (one output per lane: fine_fuzz_gen's note)
    for kind in ("plain", "nonfinite", "subnormal"):
        assert {s.chunk > s.threads for s in seeds if s.kind == kind} == {False, True}, kind
    assert {s.n_inputs for s in seeds} == set(gen.INPUTS) == {1, 2, 3, 17, 256}
    assert {s.n_bands for s in seeds} == set(gen.BANDS)
    assert all(s.n_inputs * s.n * 8 <= gen.INPUT_BYTES_CAP and s.cost <= gen.COST_CAP for s in seeds)
    for s in seeds:
        assert len(s.inputs) == len(s.steps) == s.n_bands and set(s.inputs) <= set(s.used) and all(0 <= i < s.n_inputs for i in s.inputs)
        assert (s.spare is None) == (s.n_inputs == 1) and s.spare not in s.inputs
        if s.n_inputs >= 2:
            assert len(set(s.inputs)) < s.n_inputs, s.ident  # at least one input is read by nobody
        if s.n_bands >= 2:
            assert len(set(s.inputs)) < s.n_bands, s.ident  # several bands on one input
        assert all(g in gen.GAPS for g in s.gaps) and len(s.gaps) == 4
    assert any(s.n_inputs == 256 and 255 in s.inputs for s in seeds)
    assert {g for s in seeds for g in s.gaps[0::2]} >= {0, 4} and {g for s in seeds for g in s.gaps[1::2]} >= {0, 4}
    assert set().union(*(s.events for s in seeds)) == set(gen.EVENTS)
    assert any(s.events == set(gen.EVENTS) for s in seeds)
    for s in seeds:
        n = len(s.cuts)
        moves = sorted((c, e) for c, ev in s.changes.items() for e in ev if e[0] == "set_input")
        assert ("move" in s.events) == (len(moves) == 2)
        if moves:
            (a, there), (z, back) = moves
            assert 1 <= a < z < n and there[1] == back[1] and there[2] == s.spare and back[2] == s.inputs[there[1]] != s.spare
        for c, ev in s.changes.items():
            assert 1 <= c < n
            for name, band, value in ev:
                assert name in ("set_input", "set_nco_step") and 0 <= band < s.n_bands
                assert name != "set_nco_step" or (-32768 <= value <= 32767 and value != s.steps[band])
        assert s.switch_at is None or 1 <= s.switch_at < n
    assert any("move" in s.events and s.n_inputs >= 17 for s in seeds)


def test_default_seeds_reach_every_cut_and_edge(seeds):
    for s in seeds:
        m, d, t = s.outputs, s.d, s.t
        assert m == 2 * gen.TILE + s.chunk + 1 and sum(s.cuts) == m and min(s.cuts) >= 1 and s.n == m * d
        assert s.first % d == 0 and s.first >= 0
        assert 1 in s.cuts and s.chunk in s.cuts
        for c in (s.chunk - 1, s.chunk + 1):  # where they fit beside the calls that are always there (ddc_fuzz_gen's rule)
            assert c in s.cuts or c == 0 or 1 + s.chunk + (2 * min((t - 2) // d // 2, gen.TILE // 4) if t - 1 > 2 * d else 0) + c > m, (s.ident, c)
        if t - 1 > 2 * d:
            assert any(a == b and a * d < t - 1 for a, b in zip(s.cuts[:-1], s.cuts[1:])), s.ident
    assert any(s.short_calls >= 2 for s in seeds)
    assert {s.first_kind for s in seeds} == set(gen.FIRSTS) == {"zero", "multiple", "2^31", "2^32"}
    for edge, kind in ((2 ** 31, "2^31"), (2 ** 32, "2^32")):
        crossing = [s for s in seeds if s.first < edge < s.first + s.n]
        assert len(crossing) >= 3 and {s.first_kind for s in crossing} == {kind}


@pytest.mark.parametrize("seed", gen.seeds(), ids=lambda s: s.ident)
def test_the_reference_alone(table, seed):
    """The composed reference of the cut run is fine_ref.FineRef's, call by call with the events; without the events the cut
    run is the whole run; an event changes its band from its call on; and the streams are what their kind says."""
    s = seed
    x = s.streams()
    assert x.dtype == np.float32 and x.shape == (s.n_inputs, s.n, 2)
    same = {"bits_equal": bits_equal, "nan_equal_bits": nan_equal_bits}[s.same()]
    whole, cut = s.reference(*table, x=x)
    assert whole.shape == cut.shape == (s.n_bands, s.outputs, 2) and whole.dtype == np.float32
    assert same(s.reference_cut(*table, x), cut), "the composed reference differs from FineRef along the cuts"
    assert same(s.reference_cut(*table, x, events=False), whole), "the reference along the cuts differs from the whole stream"
    touched = {e[1] for ev in s.changes.values() for e in ev}
    others = [b for b in range(s.n_bands) if b not in touched]
    assert same(cut[others], whole[others])
    for band in touched:  # the band is the whole run's up to its first event's call and differs behind it
        at = sum(s.cuts[:min(c for c, ev in s.changes.items() if any(e[1] == band for e in ev))])
        assert same(cut[band, :at], whole[band, :at]), (s.ident, band)
        assert not same(cut[band, at:], whole[band, at:]) or s.kind == "zeros", (s.ident, band)
    tiny = np.finfo(np.float32).tiny
    if s.kind == "zeros":
        assert not x.any() and np.signbit(x).sum() > x.size // 4
        assert bits_equal(whole, np.zeros_like(whole)) and bits_equal(cut, whole), "an output word of the all-zero streams is not +0"
    elif s.kind == "nonfinite":
        assert np.isfinite(whole).mean() >= 0.5 and np.isfinite(cut).mean() >= 0.5
        assert np.isnan(whole).any() and np.isposinf(whole).any() and np.isneginf(whole).any()
        planted = ~np.isfinite(x).all(axis=2) | (np.abs(x) == dgen.FLT_MAX).any(axis=2) | (np.signbit(x) & (x == 0)).all(axis=2)
        assert (planted.sum(axis=1) == len(gen.PLANTS)).all()
    elif s.kind == "subnormal":
        assert np.all(np.abs(whole) < tiny) and np.count_nonzero(whole) > whole.size * 0.9
        assert np.all(np.abs(cut) < tiny) and np.count_nonzero(cut) > cut.size * 0.9
    else:
        assert np.isfinite(whole).all() and np.count_nonzero(whole) > whole.size * 0.9 and np.abs(whole).max() > tiny
