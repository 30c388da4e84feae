"""The 8-bit k_fft_r32 kernels' register budget, checked at compile time (no GPU), as tests/test_kernel_resources_sc16.py
checks the sc16 kernel: the instances k_fft_r32<InIq8, false> (k_fft_r32_iq8.hip) and k_fft_r32<InIq8, true>
(k_fft_r32_hop_iq8.hip) of k_fft_r32.h, device-only for gfx950 with the library's own flags, and the compiler's resource report read.  Each
kernel must run at two waves per SIMD with nothing in scratch and no spilled vector register; the strided form may keep a
scalar register in a vector register's lane, as k_fft_r32_hop does.  Each unit holds its 8-bit kernel and no other."""
import pytest

from kernel_report import kernel_report, only_kernel
from sdrainer_amd.csrc import build as hip_build

# (the mangled names of the two instances: ...k_fft_r32INS_5InIq8ELb0E<argument pack and parameters>)
UNITS = {"k_fft_r32_iq8.hip": "k_fft_r32INS_5InIq8ELb0E", "k_fft_r32_hop_iq8.hip": "k_fft_r32INS_5InIq8ELb1E"}


@pytest.fixture(scope="module", params=sorted(UNITS))
def usage(request, tmp_path_factory):
    unit, kernel = request.param, UNITS[request.param]
    assert unit in hip_build.SOURCES
    assert hip_build.EXTRA_FLAGS[unit] == hip_build.EXTRA_FLAGS["k_fft_r32.hip"]
    report = kernel_report(unit, tmp_path_factory)
    assert len(report) == 1, sorted(report)
    u = dict(only_kernel(report, kernel))
    u["hop"] = "hop" in unit
    return u


def _int(usage, key):
    assert key in usage, f"{key!r} missing from the report: {sorted(usage)}"
    return int(usage[key])


def test_no_vector_spills(usage):
    assert _int(usage, "VGPRs Spill") == 0
    if not usage["hop"]:
        assert _int(usage, "SGPRs Spill") == 0


def test_no_scratch(usage):
    assert _int(usage, "ScratchSize [bytes/lane]") == 0


def test_vgprs_and_occupancy(usage):
    assert _int(usage, "VGPRs") <= 256
    assert _int(usage, "Occupancy [waves/SIMD]") == 2
