"""The fine converter kernels' resources, checked at compile time (no GPU) in the manner of tests/test_kernel_resources_ddc.py:
k_fine.hip compiled device-only for gfx950 with the library's own flags, and the compiler's resource report read.  The unit
holds exactly its two kernels - k_fine and k_fine_carry, no instance of the down-converter's templates it includes - and
neither has a spilled register or anything in scratch.  The LDS image is dynamic and is the down-converter's (csrc/ddc.h
ddc_shape, which k_fine.hip's launcher calls): the report's static LDS and the largest image stay within the 160 KB of a
CU, and the registers leave room for at least 4 waves per SIMD."""
import os
import re

import pytest

from kernel_report import kernel_report
from sdrainer_amd.csrc import build as hip_build

UNIT = "k_fine.hip"
KERNELS = ["6k_fineE", "12k_fine_carryE"]
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    assert UNIT in hip_build.SOURCES and "capi_fine.hip" in hip_build.SOURCES
    assert "fine.h" in hip_build.HEADERS and "host/fine_tune.h" in hip_build.HEADERS
    return kernel_report(UNIT, tmp_path_factory)


def test_the_unit_holds_exactly_the_fine_kernels(report):
    assert len(report) == len(KERNELS), sorted(report)
    for k in KERNELS:
        assert sum(k in name for name in report) == 1, (k, sorted(report))
    assert not [name for name in report if "k_ddc" in name]


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_no_scratch_and_lds_within_a_cu(report, kernel):
    u = next(v for name, v in report.items() if kernel in name)
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    assert int(u["LDS Size [bytes/block]"]) <= LDS_LIMIT
    assert int(u["Occupancy [waves/SIMD]"]) >= 4


def test_the_dynamic_image_is_the_down_converters():
    """k_fine.hip asks ddc_shape for its chunk, width, threads and LDS bytes and raises its limit to kDdcMaxLdsBytes: restated
    here for the geometries' corners."""
    src = open(os.path.join(hip_build.HERE, UNIT)).read()
    assert re.search(r"const DdcShape s = ddc_shape\(l\.decimation, l\.n_taps\);", src)
    assert re.search(r"raise_lds_limit_once\(once, \{\(const void \*\)k_fine\}, kDdcMaxLdsBytes\)", src)
    assert re.search(r"dim3\(\(unsigned\)s\.threads\), s\.lds_bytes, stream", src)
    ddc = open(os.path.join(hip_build.HERE, "ddc.h")).read()
    assert re.search(r"kDdcMaxLdsBytes = 160 \* 1024;", ddc)
    fine = open(os.path.join(hip_build.HERE, "fine.h")).read()
    assert re.search(r"kFineMaxBands = kDdcMaxBands, kFineMaxInputs = 256;", fine)

    def width(c, d, t):
        return (((c - 1) * d + t + d - 1) // d) | 1

    for d in (1, 2, 3, 5, 8, 64, 100, 255, 256):
        for t in (1, 5, 64, 1024, 4095, 4096):
            c = 512
            while c > 1 and d * width(c, d, t) * 8 > LDS_LIMIT:
                c -= 1
            assert d * width(c, d, t) * 8 <= LDS_LIMIT and c >= 32, (d, t)
