"""csrc/host/nb_rule.h, the impulse noise blanker's integer rule, walked on the host by tests/host/nb_rule_main.cpp (no HIP,
no library, no GPU): the per-block threshold the kernels compare with decides exactly what the defining inequality
decides, the extreme values stay inside 64 bits, and the plain C++ form of the definition blanks what it should in every
format."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_nb_rule_on_the_host(tmp_path):
    exe = str(tmp_path / "nb_rule_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "nb_rule_main.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.split() == ["nb", "rule", "ok"], p.stdout + p.stderr
