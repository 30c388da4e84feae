"""host::widen_frame (csrc/host/delivery.h), the one place the host widens a 32-bit frame word: a stand-alone C++ program,
no GPU and no library (tests/host/test_widen_frame.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_widen_frame_inverts_the_cast(tmp_path):
    """Frames up to 2^31 - 1 on either side of first_frame, first_frame just below and just above each multiple of 2^32 and
    of 2^31 up to 6 * 2^32; built with -fsanitize=undefined where the compiler has it (the casts are the point)."""
    src = os.path.join(ROOT, "tests", "host", "test_widen_frame.cpp")
    exe = str(tmp_path / "test_widen_frame")
    cc = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=undefined", "-fno-sanitize-recover=all", "-o", exe, src],
                        capture_output=True, text=True)
    if cc.returncode != 0 and "sanitize" in cc.stderr:
        cc = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, src], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-2000:]
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "failures 0" in out.stdout, out.stdout + out.stderr
    assert " 0 of them" not in out.stdout
