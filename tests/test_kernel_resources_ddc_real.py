"""The real-input down-converter kernels' resources, checked at compile time (no GPU) in the manner of
tests/test_kernel_resources_ddc.py: k_ddc_real.hip compiled device-only for gfx950 with the library's own flags, and the
compiler's resource report read.  The unit holds exactly its instances - k_ddc over the three real input traits (float,
int16 and byte word) and k_ddc_carry over the one-byte word - each with no spilled register, nothing in scratch, static LDS
within the 160 KB of a CU (the image is dynamic: tests/test_kernel_resources_ddc.py restates its size) and registers that
leave room for at least four waves per SIMD."""
import os

import pytest

from kernel_report import kernel_report
from sdrainer_amd.csrc import build as hip_build

UNIT = "k_ddc_real.hip"
KERNELS = ["k_ddcINS_9InRealF32E", "k_ddcINS_9InRealS16E", "k_ddcINS_7InReal8E", "k_ddc_carryIhE"]
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    assert UNIT in hip_build.SOURCES and "k_ddc.h" in hip_build.HEADERS and "host/ddc_format.h" in hip_build.HEADERS
    return kernel_report(UNIT, tmp_path_factory)


def test_the_unit_holds_exactly_the_real_ddc_kernels(report):
    assert len(report) == len(KERNELS), sorted(report)
    for k in KERNELS:
        assert sum(k in name for name in report) == 1, (k, sorted(report))


def test_the_unit_is_built_into_the_library():
    assert UNIT in hip_build.SOURCES and hip_build.SOURCES.index("k_ddc.hip") < hip_build.SOURCES.index(UNIT)
    assert os.path.exists(os.path.join(hip_build.HERE, UNIT))


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_no_scratch_and_lds_within_a_cu(report, kernel):
    u = next(v for name, v in report.items() if kernel in name)
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    assert int(u["LDS Size [bytes/block]"]) <= LDS_LIMIT
    assert int(u["Occupancy [waves/SIMD]"]) >= 4  # (registers leave room for every wave the LDS image lets onto a CU)
