"""k_fft_r32's register budget, checked at compile time (no GPU): the kernel runs at two waves per SIMD with every vector
register in use, and a toolchain or source change that pushes its prefetched samples out to scratch costs 20 - 30 % of
the kernel without changing a single result.  The kernel is compiled device-only for gfx950 with the library's own
flags (sdrainer_amd/csrc/build.py) and the compiler's resource report is read."""
import os
import subprocess

import pytest

from kernel_report import kernel_report, only_kernel
from sdrainer_amd.csrc import build as hip_build

UNIT = "k_fft_r32.hip"


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    # the instance k_fft_r32<InF32, false> (its mangled name: ...k_fft_r32INS_5InF32ELb0E...)
    return only_kernel(kernel_report(UNIT, tmp_path_factory), "k_fft_r32INS_5InF32ELb0E")


def _int(usage, key):
    assert key in usage, f"{key!r} missing from the report: {sorted(usage)}"
    return int(usage[key])


def test_no_spills(usage):
    assert _int(usage, "VGPRs Spill") == 0
    assert _int(usage, "SGPRs Spill") == 0


def test_no_scratch(usage):
    assert _int(usage, "ScratchSize [bytes/lane]") == 0


def test_vgprs_and_occupancy(usage):
    assert _int(usage, "VGPRs") <= 256
    assert _int(usage, "Occupancy [waves/SIMD]") == 2


def test_lds_fits():
    """The LDS is dynamic (the report says 0): the kernel's own constant kLdsBytes, evaluated by the compiler."""
    probe = ('#include "k_fft_r32.h"\n'
             'static_assert(sdr::r32::kLdsBytes <= 160 * 1024, "k_fft_r32 needs more LDS than a CU has");\n')
    cc = hip_build.hipcc()
    p = subprocess.run([cc] + hip_build.FLAGS + hip_build.EXTRA_FLAGS.get("k_fft_r32.hip", []) +
                       ["--cuda-device-only", "-fsyntax-only", "-I", hip_build.HERE, "-x", "hip", "-"],
                       input=probe, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
