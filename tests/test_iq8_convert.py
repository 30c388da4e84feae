"""8-bit input's conversions and staging image, checked on the CPU (no GPU): sdrainer_amd/csrc/iq8.h is compiled as host
code by tests/host/test_iq8_host.cpp (g++ -ffp-contract=off, like the library) - the very functions the kernels run.

* iq8::re_of / im_of equal the exact rationals x / 128 (cs8) and (2 x - 255) / 256 (cu8) for all 256 inputs, in the I and
  in the Q byte of a sample word;
* k_fft_psd_iq8's LDS staging image is a bijection, its DMA rows read exactly their own bytes, the pass-0 reads find their
  samples, and the 32 lanes of every half of a 16-bit read touch 32 different banks or share a dword (N = 512 ... 16384);
* the values the host program prints are the ones the GPU tests' bank A is fed (tests/iq8_tools.py to_f32)."""
import os
import subprocess

import numpy as np
import pytest

import iq8_tools as t8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_iq8_host.cpp")


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("iq8") / "test_iq8_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


def test_conversion_and_image(host_run):
    assert host_run.strip().splitlines()[-1] == "ok"


@pytest.mark.parametrize("fmt", t8.FORMATS, ids=t8.FORMAT_IDS)
def test_conversion_is_what_the_tests_feed_bank_a(host_run, fmt):
    name = t8.FORMAT_IDS[fmt]
    line = next(ln for ln in host_run.splitlines() if ln.startswith(name + ":"))
    host = np.array([float.fromhex(x) for x in line.split()[1:]], np.float64)
    x = np.arange(-128, 128).astype(np.int8) if fmt == t8.CS8 else np.arange(256).astype(np.uint8)
    want = t8.to_f32(x, fmt)
    assert host.size == 256
    assert np.array_equal(host.astype(np.float32).view(np.uint32), want.view(np.uint32))
    exact = np.arange(-128, 128) / 128.0 if fmt == t8.CS8 else (2.0 * np.arange(256) - 255.0) / 256.0
    assert np.array_equal(host, exact)
