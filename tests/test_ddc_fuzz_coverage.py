"""What the default seeds of tests/test_ddc_fuzz_gpu.py reach, proved without a GPU: tests/host/ddc_shape_probe.cpp prints
sdr::ddc_shape of the library's own header (plain and under AddressSanitizer and UBSan), so the nine (chunk, threads) tile
shapes the kernel can take, and the shape of every seed, are the launcher's and not a restatement; the seeds reach every
shape with every input format, every band count, value kind and entry point, a retune, a stream switch, sample indices
across 2^31 and 2^32, calls shorter than the carry and the largest LDS image; and the reference alone, run over every seed,
agrees with itself along the cuts, holds the conditions of the non-finite and the all-zero streams, and stays within the
cost cap."""
import os
import subprocess

import numpy as np
import pytest

import ddc_fuzz_gen as gen
import ddc_ref as R
from parity_tools import bits_equal, capi, nan_equal_bits  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "ddc_shape_probe.cpp")
TAP_COUNTS = (1, 5, 64, 1024, 4095, 4096)  # those of test_kernel_resources_ddc.py


def hip_include():
    """The HIP headers that ddc.h includes: beside the compiler the library is built with."""
    from sdrainer_amd.csrc import build as hip_build

    try:
        cc = hip_build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    roots = [os.path.dirname(os.path.dirname(p)) for p in (cc, os.path.realpath(cc))] + [os.environ.get("ROCM_PATH"), "/opt/rocm"]
    for root in roots:
        if root and os.path.isfile(os.path.join(root, "include", "hip", "hip_runtime.h")):
            return os.path.join(root, "include")
    pytest.fail("no include/hip/hip_runtime.h beside " + cc)


def build_probe(tmp, sanitizer):
    exe = str(tmp / ("ddc_shape_probe" + ("_san" if sanitizer else "")))
    flags = [f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all"] if sanitizer else []
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I" + hip_include()]
                        + flags + ["-o", exe, SRC], capture_output=True, text=True)
    if sanitizer and cc.returncode != 0 and "sanitize" in cc.stderr and "error:" not in cc.stderr.replace("-Werror", ""):
        pytest.skip("this compiler has no -fsanitize=" + sanitizer)
    assert cc.returncode == 0, cc.stderr
    return exe


def ask(exe, *args):
    """{(D, T): (chunk, threads, width, lds_bytes)}"""
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and not run.stderr, run.stdout[-2000:] + run.stderr[-2000:]
    rows = [[int(w) for w in line.split()] for line in run.stdout.splitlines()]
    return {(r[0], r[1]): tuple(r[2:]) for r in rows}


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return build_probe(tmp_path_factory.mktemp("ddc_shape"), None)


@pytest.fixture(scope="module")
def seeds():
    return gen.seeds()


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


@pytest.mark.parametrize("sanitizer", [None, "address,undefined"])
def test_the_probe_and_the_generator_agree_on_every_shape(tmp_path, seeds, sanitizer):
    exe = build_probe(tmp_path, sanitizer)
    grid = ask(exe, "grid", *TAP_COUNTS)
    assert len(grid) == gen.MAX_D * len(TAP_COUNTS)
    for (d, t), s in grid.items():
        assert s == gen.shape(d, t), (d, t)
    assert {s[:2] for s in grid.values()} == set(gen.CLASSES) and len(gen.CLASSES) == 9
    pairs = sorted({(s.d, s.t) for s in seeds} | {g for _, examples in gen.TABLE for g in examples})
    asked = ask(exe, *[x for p in pairs for x in p])
    for p in pairs:
        assert asked[p] == gen.shape(*p), p
    for cls, examples in gen.TABLE:
        assert all(asked[g][:2] == cls for g in examples), cls
    assert subprocess.run([exe, "257", "1"], capture_output=True).returncode == 1  # (outside the library's limits: refused)
    assert gen.TILE == int(open(os.path.join(ROOT, "include", "sdrainer_hip.h")).read().split("#define SDR_DDC_TILE_OUTPUTS ")[1].split()[0])


def test_default_seeds_reach_every_shape_with_every_format(probe, seeds):
    assert len(seeds) == gen.DEFAULT_SEEDS == 36
    shapes = ask(probe, *[x for s in seeds for x in (s.d, s.t)])
    for s in seeds:
        assert shapes[(s.d, s.t)] == (s.chunk, s.threads, s.width, s.lds_bytes), s.ident
    reachable = {v[:2] for v in ask(probe, "grid", *TAP_COUNTS).values()}
    assert {s.cls for s in seeds} == reachable and len(reachable) == 9
    assert {(s.cls, s.fmt) for s in seeds} == {(c, f) for c in reachable for f in R.FORMATS}
    # both kinds of example geometry where a class has two: T - 1 well below D * chunk, and T near 4096
    for cls, examples in gen.TABLE:
        assert {(s.d, s.t) for s in seeds if s.cls == cls} == set(examples), cls
    assert len({s.ident for s in seeds}) == len(seeds)


def test_default_seeds_reach_every_band_count_kind_and_entry_point(seeds):
    assert {s.n_bands for s in seeds} == set(gen.BANDS) == {1, 2, 3, 7, 64}
    assert {s.kind for s in seeds} == set(gen.KINDS)
    for s in seeds:
        assert s.kind != "nonfinite" or s.fmt == R.F32
        assert s.kind != "full_scale" or s.fmt != R.F32
        assert s.kind != "zeros" or s.fmt != R.CU8  # (cu8 has no zero sample)
        assert len(s.steps) == s.n_bands and all(-32768 <= x <= 32767 for x in s.steps)
    assert {k for s in seeds for k in s.entries} == {"device", "host"} == {s.whole_entry for s in seeds}
    assert any(len(set(s.entries)) == 2 for s in seeds)  # host and device calls mixed in one stream
    steps = {x for s in seeds for x in s.steps}
    assert set(gen.STEPS) <= steps and len(steps - set(gen.STEPS)) >= 10
    # the all-zero streams of the table sit where a lane has one output (ddc_fuzz_gen's note); every other kind on both sides
    for kind in ("plain", "nonfinite", "full_scale"):
        assert {s.chunk > s.threads for s in seeds if s.kind == kind} == {False, True}, kind


def test_default_seeds_reach_every_event_and_edge(seeds):
    assert any(s.retune for s in seeds) and any(not s.retune for s in seeds)
    assert any(s.switch_at for s in seeds) and any(s.retune and s.switch_at for s in seeds)
    for s in seeds:
        m, d, t = s.outputs, s.d, s.t
        assert m == 2 * gen.TILE + s.chunk + 1 <= 1537 and sum(s.cuts) == m and min(s.cuts) >= 1 and len(s.entries) == len(s.cuts)
        assert s.first % d == 0 and s.first >= 0
        assert 1 in s.cuts and s.chunk in s.cuts
        for c in (s.chunk - 1, s.chunk + 1):  # where they fit beside the calls that are always there
            assert c in s.cuts or c == 0 or 1 + s.chunk + (2 * min((t - 2) // d // 2, gen.TILE // 4) if t - 1 > 2 * d else 0) + c > m, (s.ident, c)
        if t - 1 > 2 * d:
            assert any(a == b and a * d < t - 1 for a, b in zip(s.cuts[:-1], s.cuts[1:])), s.ident
        assert s.retune is None or (1 <= s.retune[0] < len(s.cuts) and 0 <= s.retune[1] < s.n_bands and s.retune[2] != s.steps[s.retune[1]])
        assert s.switch_at is None or 1 <= s.switch_at < len(s.cuts)
    for edge in (2 ** 31, 2 ** 32):
        crossing = [s for s in seeds if s.first < edge < s.first + s.outputs * s.d]
        assert len(crossing) >= 4 and {s.first_kind for s in crossing} == {"2^31" if edge == 2 ** 31 else "2^32"}
        # and a call, not only the run, has the edge inside it
        assert any(a < edge < e for s in crossing for a, e in zip(s.first + np.cumsum([0] + s.cuts[:-1]) * s.d, s.first + np.cumsum(s.cuts) * s.d))
    assert {s.first_kind for s in seeds} == set(gen.FIRSTS)
    assert any(s.short_calls >= 2 for s in seeds)
    assert max(s.lds_bytes for s in seeds) >= 163_000 and all(s.lds_bytes <= gen.MAX_LDS for s in seeds)
    assert all(s.cost <= gen.COST_CAP for s in seeds)


@pytest.mark.parametrize("seed", gen.seeds(), ids=lambda s: s.ident)
def test_the_reference_alone(table, seed):
    """Cut and whole agree bit for bit (before a retune; from it on the retuned band, and only that band, differs), and the
    streams are what their kind says."""
    s = seed
    assert s.cost == s.n_bands * s.t * s.outputs <= gen.COST_CAP
    raw = s.raw()
    assert raw.dtype == R.RAW_DTYPE[s.fmt] and raw.shape == (s.outputs * s.d, 2)
    x = R.to_f32(raw, s.fmt)
    same = {"bits_equal": bits_equal, "nan_equal_bits": nan_equal_bits}[s.same()]
    whole, want_cut = s.reference(*table, raw=raw)
    assert whole.shape == (s.n_bands, s.outputs, 2) and whole.dtype == np.float32
    cut = s.reference_cut(*table, x, retune=False)
    assert same(cut, whole), "the reference along the cuts differs from the whole stream"
    if s.retune:
        call, band, _ = s.retune
        at = sum(s.cuts[:call])
        others = [b for b in range(s.n_bands) if b != band]
        assert same(want_cut[others], whole[others]) and same(want_cut[:, :at], whole[:, :at])
        assert not same(want_cut[band, at:], whole[band, at:]) or s.kind == "zeros"
        assert same(want_cut[band], s.reference_cut(*table, x, bands=[band])[0])
    else:
        assert want_cut is whole
    if s.kind == "zeros":
        assert not raw.any() and bits_equal(whole, np.zeros_like(whole)), "an output word of the all-zero stream is not +0"
        assert s.fmt != R.F32 or np.signbit(raw).sum() > raw.size // 4
    elif s.kind == "nonfinite":
        assert np.isfinite(whole).mean() >= 0.5
        assert np.isnan(whole).any() and np.isposinf(whole).any() and np.isneginf(whole).any()
        planted = ~np.isfinite(raw).all(axis=1) | (np.abs(raw) == gen.FLT_MAX).any(axis=1) | (np.signbit(raw) & (raw == 0)).all(axis=1)
        assert planted.sum() == len(gen.PLANTS)
    elif s.kind == "full_scale":
        info = np.iinfo(raw.dtype)
        assert ((raw == info.min) | (raw == info.max)).all(axis=1).sum() >= 12
        assert np.isfinite(whole).all()
    else:
        assert np.isfinite(whole).all() and np.count_nonzero(whole) > whole.size * 0.9
