"""The channelizer kernels' resources, checked at compile time (no GPU) in the manner of tests/test_kernel_resources_ddc.py:
k_chan.hip compiled device-only for gfx950 with the library's own flags, and the compiler's resource report read.  Every
instance - k_chan over the three complex and the three real input traits - has no spilled register and nothing in scratch.
The LDS is dynamic (span and image, csrc/chan.h): the report's static LDS and the size the launcher asks for stay within
the 160 KB of a CU for every legal geometry, sdr_chan_tile_outputs is what the restated shape says, and it is at least 16."""
import os
import re

import pytest

from kernel_report import kernel_report
from sdrainer_amd.csrc import build as hip_build

UNIT = "k_chan.hip"
KERNELS = ["k_chanINS_5InF32E", "k_chanINS_6InSc16E", "k_chanINS_5InIq8E", "k_chanINS_9InRealF32E", "k_chanINS_9InRealS16E", "k_chanINS_7InReal8E"]
LDS_LIMIT = 160 * 1024


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    assert UNIT in hip_build.SOURCES and "capi_chan.hip" in hip_build.SOURCES
    assert all(h in hip_build.HEADERS for h in ("chan.h", "k_chan.h", "ddc_input_real.h", "front_input.h", "host/nco_table.h"))
    return kernel_report(UNIT, tmp_path_factory)


def test_the_unit_holds_exactly_the_channelizer_kernels(report):
    assert len(report) == len(KERNELS), sorted(report)
    for k in KERNELS:
        assert sum(k in name for name in report) == 1, (k, sorted(report))


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_spills_no_scratch_and_lds_within_a_cu(report, kernel):
    u = next(v for name, v in report.items() if kernel in name)
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    assert int(u["LDS Size [bytes/block]"]) <= LDS_LIMIT
    assert int(u["Occupancy [waves/SIMD]"]) >= 4  # (registers leave room for every wave the LDS lets onto a CU)


def test_the_tile_stays_within_a_cu_for_every_geometry():
    """csrc/chan.h restated: R = 4096 / M output times per workgroup, a span of (R - 1) D + T pairs and an image of
    R (M + 1) pairs, 8 bytes each."""
    from sdrainer_amd import capi

    src = open(os.path.join(hip_build.HERE, "chan.h")).read()
    assert re.search(r"kChanMaxLdsBytes = 160 \* 1024;", src) and re.search(r"kChanThreads = 256;", src)
    assert re.search(r"kChanLogItems = 12, kChanTileItems = 1 << kChanLogItems;", src)
    seen = 0
    for log_m in range(1, 9):
        m = 1 << log_m
        for d in (m, m // 2, m // 4):
            if d < 1:
                continue
            for p in range(1, 65):
                t = p * m
                if t > 4096:
                    assert capi.chan_tile_outputs(m, d, t) < 0
                    continue
                tile = capi.chan_tile_outputs(m, d, t)
                assert tile == 4096 // m and tile >= 16, (m, d, t, tile)
                assert ((tile - 1) * d + t + tile * (m + 1)) * 8 <= LDS_LIMIT, (m, d, t)
                seen += 1
    assert seen > 500
    worst = (15 * 64 + 4096 + 16 * 257) * 8  # M = 256, D = 64, T = 4096: about 72 KB
    assert 72_000 <= worst <= 74_000
