"""The IQ-correction units' resources, checked at compile time (no GPU) in the manner of tests/test_kernel_resources_chan.py:
k_ddc_iqc.hip, k_chan_iqc.hip and k_iq_sums.hip compiled device-only for gfx950 with the library's own flags, and the
compiler's resource report read.  Each unit holds exactly its instances - k_ddc and k_chan over the three corrected traits,
the two sums kernels and their finishing pass - with no spilled register and nothing in scratch; the corrected kernels keep
the occupancy of the uncorrected ones, and the sums kernels' static LDS is the four waves' totals."""
import os
import re
import subprocess

import pytest

from sdrainer_amd.csrc import build as hip_build

UNITS = {
    "k_ddc_iqc.hip": ["k_ddcINS_11InCorrectedINS_5InF32EEE", "k_ddcINS_11InCorrectedINS_6InSc16EEE", "k_ddcINS_11InCorrectedINS_5InIq8EEE"],
    "k_chan_iqc.hip": ["k_chanINS_11InCorrectedINS_5InF32EEE", "k_chanINS_11InCorrectedINS_6InSc16EEE", "k_chanINS_11InCorrectedINS_5InIq8EEE"],
    "k_iq_sums.hip": ["k_iq_sums_iq8E", "k_iq_sums_sc16E", "k_iq_sums_finishE"],
}
CASES = [(u, k) for u, ks in UNITS.items() for k in ks]


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    try:
        cc = hip_build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    assert all(u in hip_build.SOURCES for u in UNITS)
    assert all(h in hip_build.HEADERS for h in ("iq_correct.h", "iq_sums_dev.h", "host/iq_sums.h"))
    tmp = tmp_path_factory.mktemp("res")
    out = {}
    for unit in UNITS:
        cmd = [cc] + hip_build.FLAGS + hip_build.EXTRA_FLAGS.get(unit, []) + ["--cuda-device-only", "-c", os.path.join(hip_build.HERE, unit), "-o",
                                                                             str(tmp / unit.replace(".hip", ".o")), "-Rpass-analysis=kernel-resource-usage"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-4000:]
        usage = {}
        for name, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", p.stderr, re.S):
            usage[name] = {k.strip(): v for k, v in re.findall(r"remark: +([A-Za-z][A-Za-z /\[\]]*?): (\S+)", body)}
        out[unit] = usage
    return out


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
