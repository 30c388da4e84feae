"""The impulse noise blanker's kernels' resources, checked at compile time (no GPU) in the manner of
tests/test_kernel_resources_iqc.py: k_nb.hip compiled device-only for gfx950 with the library's own flags, and the
compiler's resource report read.  The unit holds exactly its ten kernels - the power pass per sample type, the gate pass per
format, the carry pass - with no spilled register and nothing in scratch.  The expected figures are the design's
(csrc/k_nb.hip, nb.h): the power pass keeps one 8-byte sum per 64-byte block of a 16 KB tile in LDS, the gate pass one
4-byte threshold per block and for the block in front, the lookback's last impulse, the four waves' and their two counts,
the carry pass its two 8-byte totals; both streaming passes are memory-bound and want every wave slot, which 64 VGPRs or
fewer and a 256-thread workgroup give: 8 waves per SIMD."""
import os

import pytest

from kernel_report import kernel_report
from sdrainer_amd.csrc import build as hip_build

UNIT = "k_nb.hip"
SC16, CS8, CU8, REAL = 1, 2, 3, 16
POWER = [f"k_nb_powerILi{b}EE" for b in (SC16, CS8, CU8)]
GATE = [f"k_nb_gateILi{f}EE" for f in (SC16, CS8, CU8, REAL | SC16, REAL | CS8, REAL | CU8)]
CARRY = ["k_nb_carryE"]
TILE_BYTES, MIN_BLOCK_BYTES, WAVES = 16384, 64, 4
TILE_BLOCKS = TILE_BYTES // MIN_BLOCK_BYTES


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    assert UNIT in hip_build.SOURCES and "capi_nb.hip" in hip_build.SOURCES
    assert all(h in hip_build.HEADERS for h in ("nb.h", "host/nb_rule.h"))
    return kernel_report(UNIT, tmp_path_factory)


def test_the_unit_holds_exactly_its_kernels(report):
    assert len(report) == len(POWER + GATE + CARRY), sorted(report)
    for k in POWER + GATE + CARRY:
        assert sum(k in name for name in report) == 1, (k, sorted(report))


@pytest.mark.parametrize("kernel", POWER + GATE + CARRY)
def test_no_spills_no_scratch_and_the_designed_lds_and_occupancy(report, kernel):
    u = next(v for name, v in report.items() if kernel in name)
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    lds = TILE_BLOCKS * 8 if kernel in POWER else (TILE_BLOCKS + 1) * 4 + 4 + WAVES * 4 + WAVES * 2 * 4 if kernel in GATE else 2 * 8
    assert int(u["LDS Size [bytes/block]"]) == lds
    assert int(u["VGPRs"]) <= 64 and int(u["Occupancy [waves/SIMD]"]) == 8
