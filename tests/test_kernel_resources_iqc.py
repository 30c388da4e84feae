"""The IQ-correction units' resources, checked at compile time (no GPU) in the manner of tests/test_kernel_resources_chan.py:
k_ddc_iqc.hip, k_chan_iqc.hip and k_iq_sums.hip compiled device-only for gfx950 with the library's own flags, and the
compiler's resource report read.  Each unit holds exactly its instances - k_ddc and k_chan over the three corrected traits,
the two sums kernels and their finishing pass - with no spilled register and nothing in scratch; the corrected kernels keep
the occupancy of the uncorrected ones, and the sums kernels' static LDS is the four waves' totals."""
import pytest

from kernel_report import kernel_report
from sdrainer_amd.csrc import build as hip_build

UNITS = {
    "k_ddc_iqc.hip": ["k_ddcINS_11InCorrectedINS_5InF32EEE", "k_ddcINS_11InCorrectedINS_6InSc16EEE", "k_ddcINS_11InCorrectedINS_5InIq8EEE"],
    "k_chan_iqc.hip": ["k_chanINS_11InCorrectedINS_5InF32EEE", "k_chanINS_11InCorrectedINS_6InSc16EEE", "k_chanINS_11InCorrectedINS_5InIq8EEE"],
    "k_iq_sums.hip": ["k_iq_sums_iq8E", "k_iq_sums_sc16E", "k_iq_sums_finishE"],
}
CASES = [(u, k) for u, ks in UNITS.items() for k in ks]


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    assert all(u in hip_build.SOURCES for u in UNITS)
    assert all(h in hip_build.HEADERS for h in ("iq_correct.h", "iq_sums_dev.h", "host/iq_sums.h"))
    return {unit: kernel_report(unit, tmp_path_factory) for unit in UNITS}


@pytest.mark.parametrize("unit", list(UNITS))
def test_each_unit_holds_exactly_its_kernels(reports, unit):
    report = reports[unit]
    assert len(report) == len(UNITS[unit]), sorted(report)
    for k in UNITS[unit]:
        assert sum(k in name for name in report) == 1, (k, sorted(report))


@pytest.mark.parametrize("unit,kernel", CASES)
def test_no_spills_and_no_scratch(reports, unit, kernel):
    u = next(v for name, v in reports[unit].items() if kernel in name)
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0
    assert int(u["ScratchSize [bytes/lane]"]) == 0
    if unit == "k_iq_sums.hip":
        assert int(u["LDS Size [bytes/block]"]) == 4 * 5 * 8  # four waves' five totals
        assert int(u["Occupancy [waves/SIMD]"]) == 8
    else:
        assert int(u["LDS Size [bytes/block]"]) == 0  # (dynamic: the launcher's, as for the uncorrected kernels)
        assert int(u["Occupancy [waves/SIMD]"]) >= 4
