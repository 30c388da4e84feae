"""k_fft_r32_sc16's register budget, checked at compile time (no GPU), as tests/test_kernel_resources.py checks the
float32 kernel: the instance k_fft_r32<InSc16, false> of k_fft_r32.h (k_fft_r32_sc16.hip), device-only for gfx950 with the
library's own flags, and the compiler's resource report read.  The sc16 kernel must run at two waves per SIMD with
nothing in scratch, like the float32 one; its prefetched frame is 32 registers instead of 64."""
import pytest

from kernel_report import kernel_report, only_kernel
from sdrainer_amd.csrc import build as hip_build

UNIT = "k_fft_r32_sc16.hip"
KERNEL = "k_fft_r32INS_6InSc16ELb0E"  # (the mangled name of k_fft_r32<InSc16, false>: ...k_fft_r32INS_6InSc16ELb0E...)


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    assert UNIT in hip_build.SOURCES
    assert hip_build.EXTRA_FLAGS[UNIT] == hip_build.EXTRA_FLAGS["k_fft_r32.hip"]
    report = kernel_report(UNIT, tmp_path_factory)
    assert not any("k_fft_r32" in n and KERNEL not in n for n in report), sorted(report)
    return only_kernel(report, KERNEL)


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
