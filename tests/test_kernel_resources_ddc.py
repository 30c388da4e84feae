"""The down-converter kernels' resources, checked at compile time (no GPU) in the manner of tests/test_kernel_resources_iq8.py:
k_ddc.hip compiled device-only for gfx950 with the library's own flags, and the compiler's resource report read.  Every
instance - k_ddc over the three input traits, k_ddc_carry over the three sample words - has no spilled register and nothing
in scratch.  The LDS image is dynamic (its size follows the decimation and the tap count, csrc/ddc.h): the report's static
LDS and the largest image the launcher may ask for both stay within the 160 KB of a CU, and the tile constants of the
header, the binding and the kernel agree."""
import os
import re

import pytest

from kernel_report import kernel_report
from sdrainer_amd.csrc import build as hip_build

UNIT = "k_ddc.hip"
KERNELS = ["k_ddcINS_5InF32E", "k_ddcINS_6InSc16E", "k_ddcINS_5InIq8E", "k_ddc_carryI15HIP_vector_typeIfLj2EE", "k_ddc_carryIjE", "k_ddc_carryItE"]
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    assert UNIT in hip_build.SOURCES and "capi_ddc.hip" in hip_build.SOURCES and "ddc.h" in hip_build.HEADERS and "front_input.h" in hip_build.HEADERS
    return kernel_report(UNIT, tmp_path_factory)


def test_the_unit_holds_exactly_the_ddc_kernels(report):
    assert len(report) == len(KERNELS), sorted(report)
    for k in KERNELS:
        assert sum(k in name for name in report) == 1, (k, sorted(report))


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_no_scratch_and_lds_within_a_cu(report, kernel):
    u = next(v for name, v in report.items() if kernel in name)
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    assert int(u["LDS Size [bytes/block]"]) <= LDS_LIMIT
    assert int(u["Occupancy [waves/SIMD]"]) >= 4  # (registers leave room for every wave the LDS image lets onto a CU)


def test_the_dynamic_image_stays_within_a_cu():
    """csrc/ddc.h: the launcher asks for D * width * 8 bytes, capped by kDdcMaxLdsBytes - restated here for every (D, T)."""
    src = open(os.path.join(hip_build.HERE, "ddc.h")).read()
    assert re.search(r"kDdcMaxLdsBytes = 160 \* 1024;", src) and re.search(r"kDdcTileOutputs = SDR_DDC_TILE_OUTPUTS;", src)
    assert re.search(r"kDdcMaxThreads = 256;", src)
    header = open(os.path.join(os.path.dirname(os.path.dirname(hip_build.HERE)), "include", "sdrainer_hip.h")).read()
    tile = int(re.search(r"#define SDR_DDC_TILE_OUTPUTS (\d+)", header).group(1))

    def width(c, d, t):
        return (((c - 1) * d + t + d - 1) // d) | 1

    for d in (1, 2, 3, 5, 8, 64, 100, 255, 256):
        for t in (1, 5, 64, 1024, 4095, 4096):
            c = tile
            while c > 1 and d * width(c, d, t) * 8 > LDS_LIMIT:
                c -= 1
            assert d * width(c, d, t) * 8 <= LDS_LIMIT, (d, t)
            assert c >= 32, (d, t)  # (D = 256, T = 4096: 64 outputs, a whole wave; odd D beside it a few less)
