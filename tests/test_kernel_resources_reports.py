"""The report kernels' resources, checked at compile time (no GPU) through tools/kernel_resources.sh: k_report_marks and
k_listen_report (sdrainer_amd/csrc/k_report.hip) use no scratch and spill nothing, and the listing of the units around them -
the gather and the decoder (k_listen.hip), the pack kernels (k_results.hip) - is line for line the one kept in
profiles/reports_kernel_resources.txt, which is the parent commit's for every kernel that existed there."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTING = os.path.join(ROOT, "profiles", "reports_kernel_resources.txt")
UNITS = ("k_report", "k_listen", "k_results")


def kept():
    """{unit: [lines]} of the committed listing."""
    out, unit = {}, None
    with open(LISTING) as f:
        for line in f:
            line = line.rstrip("\n")
            if line.startswith("## "):
                unit = line[3:].replace(".hip", "")
                out[unit] = []
            elif unit and line and not line.startswith("#"):
                out[unit].append(line)
    return out


@pytest.fixture(scope="module", params=UNITS)
def listing(request):
    from sdrainer_amd.csrc import build as hip_build
    try:
        hip_build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join("sdrainer_amd", "csrc", request.param + ".hip")],
                       cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and "error" not in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    return request.param, [line for line in p.stdout.splitlines() if line.strip()]


def test_listing_is_the_kept_one(listing):
    unit, lines = listing
    assert lines == kept()[unit], f"{unit}.hip: the compiler's listing differs from profiles/reports_kernel_resources.txt"


def test_report_kernels_use_no_scratch_and_spill_nothing(listing):
    unit, lines = listing
    if unit != "k_report":
        return  # (the new kernels live in k_report.hip; the other units are held to the kept listing above)
    found = {}
    for line in lines:
        m = re.match(r"(\S+)\s+vgpr\s+(\d+)\s+agpr\s+(\d+)\s+sgpr\s+(\d+)\s+scratch\s+(\d+)\s+spill\(v/s\)\s+(\d+)/(\d+)\s+occ\s+(\d+)\s+lds\s+(\d+)", line)
        assert m, line
        found[m.group(1)] = [int(x) for x in m.groups()[1:]]
    marks = [v for k, v in found.items() if "k_report_marks" in k]
    report = [v for k, v in found.items() if "k_listen_report" in k]
    assert len(marks) == 1 and len(report) == 1 and len(found) == 2, sorted(found)
    for vgpr, agpr, sgpr, scratch, spill_v, spill_s, occ, lds in marks + report:
        assert scratch == 0 and spill_v == 0 and spill_s == 0, (vgpr, scratch, spill_v, spill_s)
    assert report[0][7] <= 65536 and report[0][6] >= 2  # its tables and partial sums fit the 64 KB a workgroup may have
