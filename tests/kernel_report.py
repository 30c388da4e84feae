"""The compiler's resource report of one unit of the library, for the compile-time tests/test_kernel_resources*.py (no GPU):
the unit compiled device-only for gfx950 with the library's own flags (build.FLAGS + EXTRA_FLAGS) and the remarks of
-Rpass-analysis=kernel-resource-usage read.  A plain module: each test module keeps its own fixture, kernel lists and
thresholds."""
import os
import re
import subprocess

import pytest

from sdrainer_amd.csrc import build as hip_build


def kernel_report(unit, tmp_path_factory):
    """{mangled kernel name: {field: value}} of every kernel in `unit` (a name of build.SOURCES); values are the report's text."""
    try:
        cc = hip_build.hipcc()
    except RuntimeError as e:
        pytest.fail(str(e))
    assert unit in hip_build.SOURCES
    out = tmp_path_factory.mktemp("res") / unit.replace(".hip", ".o")
    cmd = [cc] + hip_build.FLAGS + hip_build.EXTRA_FLAGS.get(unit, []) + ["--cuda-device-only", "-c", os.path.join(hip_build.HERE, unit), "-o", str(out),
                                                                        "-Rpass-analysis=kernel-resource-usage"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    usage = {}
    for name, body in re.findall(r"Function Name: (\S+)(.*?)(?=Function Name:|\Z)", p.stderr, re.S):
        usage[name] = {k.strip(): v for k, v in re.findall(r"remark: +([A-Za-z][A-Za-z /\[\]]*?): (\S+)", body)}
    return usage


def only_kernel(report, kernel):
    """The fields of the one kernel of `report` whose mangled name contains `kernel`."""
    found = [v for name, v in report.items() if kernel in name]
    assert len(found) == 1, f"no single resource report for {kernel}: {sorted(report)}"
    return found[0]
