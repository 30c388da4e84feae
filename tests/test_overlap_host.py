"""Overlapped frames (sdr_config.hop < block_size) without a GPU: the ABI (symbols, the header from plain C, where the hop
lies in sdr_config), the arithmetic of the staged host input (sdrainer_amd/csrc/host/overlap.h: samples and frames;
sdrainer_amd/csrc/host/staging.h: the kinds of staged frames and the bytes of their rows) and the host mirror's
clock, which one frame advances by hop / sample_rate (sdrainer_amd/csrc/host/rx.h FrameTiming)."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
NEW_SYMBOLS = ["sdr_hop", "sdr_process_device_stream", "sdr_process_device_stream_sc16"]


@pytest.fixture(scope="module")
def lib():
    from sdrainer_amd.csrc import build
    return build.build()


def test_symbols_in_library_header_and_binding(lib):
    from sdrainer_amd import capi
    dyn = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "sdrainer_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in exported, f"{name} is not exported by the library"
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in the header"
        assert name in capi.SYMBOLS
    assert re.search(r"int32_t\s+hop\s*;", header) and "int32_t reserved;\n} sdr_config;" not in header
    assert "#define SDR_ABI_VERSION 2" in header


def test_config_layout_from_plain_c(lib, tmp_path):
    """sizeof(sdr_config) stays 56 and the hop is the word that was reserved, at offset 52 - in C and in the binding."""
    from sdrainer_amd import capi
    exe = str(tmp_path / "test_overlap_layout")
    libdir = os.path.dirname(lib)
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-O1", "-o", exe, os.path.join(HOST, "test_overlap_layout.c"),
                           "-L" + libdir, "-l:" + os.path.basename(lib), "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = dict(line.rsplit(" ", 1) for line in out.stdout.strip().splitlines())
    assert got["sdr_config.hop"] == "52" and got["sizeof sdr_config"] == "56" and got["zeroed hop"] == "0" and got["abi"] == "2"
    assert capi.Config.reserved_hop.offset == 52 and C.sizeof(capi.Config) == 56
    cfg = capi.Config()
    assert cfg.hop == 0
    cfg.hop = 4096
    assert cfg.reserved_hop == 4096 and cfg.hop == 4096


@pytest.mark.parametrize("sanitizer", [None, "address,undefined"])
def test_staging_arithmetic(tmp_path, sanitizer):
    """Complete-frame count, what a batch uploads and the history it leaves, for streams pushed in pieces of 1, 3 and 7
    hops, before and after a limit cut, at hop = N, N / 2, N / 16; the hops sdr_create takes; the FFT input index."""
    exe = str(tmp_path / "test_overlap_staging")
    flags = [f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all"] if sanitizer else []
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags +
                        ["-o", exe, os.path.join(HOST, "test_overlap_staging.cpp")], capture_output=True, text=True)
    if sanitizer and cc.returncode != 0 and "sanitize" in cc.stderr and "error:" not in cc.stderr.replace("-Werror", ""):
        pytest.skip("this compiler has no -fsanitize=" + sanitizer)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.split() == ["hops", "ok", "index", "ok", "staging", "ok"]


@pytest.mark.parametrize("sanitizer", [None, "address,undefined"])
def test_staging_rows(tmp_path, sanitizer):
    """sdrainer_amd/csrc/host/staging.h: the kind table, and real bytes of all five kinds moved through the planned push,
    upload, history and leftover ranges of three staging sets, at N = 512 (hops 512, 256, 32) and 16384 (hops 16384, 1024),
    max_batch_frames 8 and 64: every batch's device rows hold the stream, every range lies inside its buffer."""
    exe = str(tmp_path / "test_staging_rows")
    flags = [f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all"] if sanitizer else []
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags +
                        ["-o", exe, os.path.join(HOST, "test_staging_rows.cpp")], capture_output=True, text=True)
    if sanitizer and cc.returncode != 0 and "sanitize" in cc.stderr and "error:" not in cc.stderr.replace("-Werror", ""):
        pytest.skip("this compiler has no -fsanitize=" + sanitizer)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout[-4000:] + run.stderr[-4000:]
    assert run.stdout.split() == ["kinds", "ok", "rows", "ok"]


@pytest.mark.parametrize("rate, n, silence", [(2_000_000, 65536, 20.0), (2_000_000, 16384, 1.0), (48_000, 512, 20.0), (192_000, 4096, 0.37)])
def test_host_mirror_clock_follows_the_hop(lib, tmp_path, rate, n, silence):
    """A silent listener with silence time-out T is detached at the first frame f with (f + 1) * hop / rate > T: at
    hop = N / k that is k times the frame of the hop = N run, up to the rounding of T * rate / hop to whole frames."""
    exe = str(tmp_path / "test_overlap_clock")
    libdir = os.path.dirname(lib)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-pthread", "-o", exe, os.path.join(HOST, "test_overlap_clock.cpp"),
                           "-L" + libdir, "-l:" + os.path.basename(lib), "-Wl,-rpath," + libdir])
    out = subprocess.run([exe, str(rate), str(n), str(silence)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    at = {int(h): int(f) for h, f in (line.split() for line in out.stdout.strip().splitlines())}
    assert sorted(at) == [n // 16, n // 4, n // 2, n]
    base = at[n]
    assert base > 0
    for k in (2, 4, 16):
        f = at[n // k]
        # (f + 1) is the smallest integer above T * rate * k / N, (base + 1) the smallest above T * rate / N
        assert k * base <= f <= k * base + (k - 1), (k, base, f)
        assert f != base
        assert f + 1 > silence * rate / (n // k) >= f  # the frame whose clock first exceeds T, by the definition itself
