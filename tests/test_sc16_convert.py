"""sc16 input's conversion and staging image, checked on the CPU (no GPU): sdrainer_amd/csrc/sc16.h is compiled as host
code by tests/host/test_sc16_host.cpp (g++ -ffp-contract=off, like the library) - the very functions the kernels run.

* sc16::to_f32 equals numpy's float32 division x / 32767 (IEEE, correctly rounded) for all 65 536 int16 values;
* k_fft_psd_sc16's LDS staging image is a bijection, its DMA rows read exactly their own bytes, the pass-0 reads find
  their samples and no ds_read_b32 lane group hits a bank twice (N = 512 ... 16384);
* the GPU test's input holds values where a plain multiply by 1/32767 rounds differently (those are the values a wrong
  conversion in a kernel would show at)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_sc16_host.cpp")


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sc16") / "test_sc16_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


def _multiply_wrong_numpy():
    v = np.arange(-32768, 32768)
    f = v.astype(np.float32)
    return v[(f * np.float32(1.0 / 32767.0)) != (f / np.float32(32767.0))]


def test_conversion_and_image(host_run):
    assert host_run.strip().splitlines()[-1] == "ok"


def test_conversion_against_numpy_division(host_run, tmp_path):
    """The host program checked against a float64 quotient; here the same functions against numpy's float32 division,
    value by value, through a dump of all 65 536 results."""
    src = tmp_path / "dump.cpp"
    src.write_text('#include <cstdio>\n#include "%s"\nint main(){for(int v=-32768;v<=32767;v++){float f=sc16::to_f32((int16_t)v);'
                   'fwrite(&f,4,1,stdout);}return 0;}\n' % os.path.join(ROOT, "sdrainer_amd", "csrc", "sc16.h"))
    exe = str(tmp_path / "dump")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, str(src)])
    got = np.frombuffer(subprocess.check_output([exe]), np.float32)
    want = np.arange(-32768, 32768).astype(np.float32) / np.float32(32767.0)
    assert got.size == 65536
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_plain_multiply_is_wrong_where_expected(host_run):
    """1 536 values round differently under x * (1/32767): the host program and numpy agree on which."""
    line = next(ln for ln in host_run.splitlines() if ln.startswith("multiply-wrong:"))
    host = np.array([int(x) for x in line.split()[1:]])
    assert len(host) == 1536
    assert np.array_equal(np.sort(host), _multiply_wrong_numpy())


def test_gpu_input_holds_multiply_wrong_values():
    pytest.importorskip("torch")
    import importlib.util
    spec = importlib.util.spec_from_file_location("sc16_gpu", os.path.join(ROOT, "tests", "test_sc16_input_gpu.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    wrong = set(_multiply_wrong_numpy().tolist())
    q, _, _ = mod.pool(512, 4, 1)
    vals = set(np.unique(q).tolist())
    assert len(vals & wrong) >= 10
    assert {32767, -32768, -32767} <= vals
