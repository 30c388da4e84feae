"""Block sizes 32768 and 65536 without a GPU: the two-phase FFT (sdrainer_amd/csrc/fft_2p.h) emulated thread by thread
against the oracle, the batch plan at the new sizes (and N = 16384 unchanged), the certified dB shortcut at log N = 15
and 16, and the new kernels' register and LDS budget on gfx950."""
import os
import re
import subprocess

import pytest

from oracle import oracle as orc
from sdrainer_amd.csrc import build as hip_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_phase_fft_matches_oracle_bit_for_bit(tmp_path):
    """k_fft_2p's phases A and B, run on the CPU with the kernels' own index and butterfly functions: psd rows equal the
    oracle's radix-2 FFT + PSD and tap values equal the psd at the listeners' bins, float32 and sc16 input, random,
    full-scale and zero frames, N = 32768 and 65536."""
    exe = str(tmp_path / "emu_fft_2p")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "emu", "emu_fft_2p.cpp"), "-ldl"])
    out = subprocess.run([exe, orc.build()], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count(": 0 mismatches, tap 0 mismatches") == 12, out.stdout


def test_batch_plan_at_wide_blocks(tmp_path):
    exe = str(tmp_path / "test_batch_plan_wide")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "test_batch_plan_wide.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0 and run.stdout.split() == ["plan", "ok"], run.stdout + run.stderr


def test_db_shortcut_certified_at_wide_blocks(tmp_path):
    """gomath.h's fast math.Log10 path with the tables of log N = 15 and 16: wherever it accepts, the reference's bits."""
    exe = str(tmp_path / "emu_log_wide")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "emu", "emu_log_wide.cpp")])
    out = subprocess.run([exe, "2000000"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "mismatches 0," in out.stdout, out.stdout + out.stderr


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    """The compiler's resource report of every kernel of k_fft_2p.hip (device-only for gfx950, the library's flags)."""
    try:
        cc = hip_build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    assert "k_fft_2p.hip" in hip_build.SOURCES
    out = tmp_path_factory.mktemp("res") / "k_fft_2p.o"
    cmd = [cc] + hip_build.FLAGS + hip_build.EXTRA_FLAGS.get("k_fft_2p.hip", []) + [
        "--cuda-device-only", "-c", os.path.join(hip_build.HERE, "k_fft_2p.hip"), "-o", str(out), "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    kernels = {}
    for m in re.finditer(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", p.stderr, re.S):
        kernels[m.group(1)] = {k.strip(): v for k, v in re.findall(r"remark: +([A-Za-z][A-Za-z /\[\]]*?): (\S+)", m.group(2))}
    return kernels


def test_two_phase_kernels_resources(usage):
    names = sorted(usage)
    # phase A is one template, k_fft2p_a<LOGN, FMT, WIN...>: the pack is mangled J..E, empty (JE) for the plain instances
    # and the window table's type for the windowed ones; N = 32768 / 65536 x float32 / sc16 of each
    phase_a = [n for n in names if "k_fft2p_a" in n]
    plain = [n for n in phase_a if re.search(r"InFormatE\dEJEE", n)]
    windowed = [n for n in phase_a if re.search(r"InFormatE\dEJ\w*PKfEE", n)]
    assert len(plain) == 4 and len(windowed) == 4 and len(phase_a) == 8, names
    assert sum("k_fft2p_b" in n for n in names) == 2 and len(names) == 10, names
    for name, u in usage.items():
        assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0, name
        assert int(u["ScratchSize [bytes/lane]"]) == 0, name
        assert int(u["LDS Size [bytes/block]"]) <= 160 * 1024, name
        assert int(u["VGPRs"]) <= 256 and int(u["Occupancy [waves/SIMD]"]) >= 2, name
        print(f"{name}: {u['VGPRs']} VGPRs, {u['LDS Size [bytes/block]']} B LDS, {u['Occupancy [waves/SIMD]']} waves/SIMD")
