"""Listener reports without a GPU: the quantisation and the NaN rule of tests/reports_ref.py at their edges, the additivity
of the reference over random cuts, the record's layout in the binding against a C11 offsetof program
(tests/host/test_reports_c.c), and the ABI facts the extension must leave alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reports_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def f32(*v):
    return np.array(v, np.float32)


def test_q_at_ties_clamps_and_specials():
    # ties go to the even neighbour: k + 0.5 quanta, exactly representable
    x = f32(0.5 / 256, 1.5 / 256, 2.5 / 256, -0.5 / 256, -1.5 / 256, 100 + 0.5 / 256, 100 + 1.5 / 256)
    assert ref.q(x).tolist() == [0, 2, 2, 0, -2, 25600, 25602]
    # just beside a tie
    assert ref.q(f32(np.nextafter(np.float32(1.5 / 256), np.float32(0)), np.nextafter(np.float32(1.5 / 256), np.float32(1)))).tolist() == [1, 2]
    # the clamps, +-Inf and -0
    assert ref.q(f32(1024, 1024.5, 3e38, np.inf, -1024, -1024.5, -3e38, -np.inf)).tolist() == [262144] * 4 + [-262144] * 4
    assert ref.q(f32(-0.0, 0.0)).tolist() == [0, 0]
    assert ref.q(f32(1023.99609375, 1023.998046875)).tolist() == [262143, 262144] and ref.q(f32(65.25)).tolist() == [16704]
    # every product is exact: q(k / 256) == k over the whole range that is not clamped
    k = np.arange(-262144, 262145, 37, dtype=np.int64)
    assert np.array_equal(ref.q((k / 256.0).astype(np.float32)), k)


def test_nan_rule():
    """A tick is measured if neither its value nor its frame's noise floor is NaN; the unmeasured ones count in ticks only."""
    nan = np.float32("nan")
    v = f32(10, nan, 30, 40, -np.inf, 60)
    nf = f32(1, 2, nan, 4, -np.inf, 6)
    d = np.array([1, 1, 1, 0, 1, 0])
    r = ref.report(v, d, nf)
    assert r == {"ticks": 6, "ticks_on": 2, "ticks_off": 2, "on_max_q": 2560, "on_sum_q": 2560 - 262144, "off_sum_q": 256 * 100,
                 "floor_sum_q": 256 - 262144}
    none = ref.report(f32(nan, 5), np.array([1, 0]), f32(1, nan))
    assert none["ticks"] == 2 and none["ticks_on"] == none["ticks_off"] == 0 and none["on_max_q"] == ref.INT32_MIN
    assert none["on_sum_q"] == none["off_sum_q"] == none["floor_sum_q"] == 0
    empty = ref.report(f32(), np.array([], np.uint8), f32())
    assert empty["ticks"] == 0 and empty["on_max_q"] == ref.INT32_MIN


def test_additivity_over_random_cuts():
    """Any cut of a stream gives the same totals: sums and counts add, on_max_q takes the maximum."""
    rng = np.random.default_rng(7)
    n = 1000
    v = (rng.normal(40, 30, n)).astype(np.float32)
    nf = (rng.normal(5, 2, n)).astype(np.float32)
    v[rng.integers(0, n, 30)] = np.nan
    nf[rng.integers(0, n, 30)] = np.nan
    v[rng.integers(0, n, 10)] = -np.inf
    v[rng.integers(0, n, 10)] = 5000
    d = rng.integers(0, 2, n)
    whole = ref.report(v, d, nf)
    assert whole["ticks_on"] > 300 and whole["ticks_off"] > 300 and whole["ticks_on"] + whole["ticks_off"] < n
    for _ in range(20):
        cuts = [0] + sorted(rng.integers(0, n + 1, rng.integers(1, 12)).tolist()) + [n]
        total = None
        for a, e in zip(cuts, cuts[1:]):
            total = ref.add(total, ref.report(v[a:e], d[a:e], nf[a:e]))
        assert total == whole, cuts


def test_snr():
    from sdrainer_amd import capi

    rec = np.zeros(2, capi.REPORT_DTYPE)
    rec[0]["ticks_on"], rec[0]["on_sum_q"], rec[0]["floor_sum_q"] = 4, 4 * 256 * 70, 4 * 256 * 5
    snr = capi.report_snr_db(rec)
    assert snr[0] == 65.0 and np.isnan(snr[1])


def test_layout_against_c(tmp_path):
    """ctypes / numpy itemsize 64 and every field's offset against offsetof in a C11 program; sdr_abi_version() stays 2 and
    sizeof(sdr_results) 128 (the program asserts both at compile time, the binding at run time)."""
    from sdrainer_amd import capi

    exe = str(tmp_path / "test_reports_c")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", "-O0", "-c", "-o", exe + ".o",
                           os.path.join(ROOT, "tests", "host", "test_reports_c.c")])
    from sdrainer_amd.csrc import build
    lib = build.build()
    libdir = os.path.dirname(lib)
    subprocess.check_call(["gcc", "-o", exe, exe + ".o", "-L" + libdir, "-l:" + os.path.basename(lib), "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    got = dict(zip(out[0::2], (int(x) for x in out[1::2])))
    assert got.pop("sizeof") == capi.REPORT_DTYPE.itemsize == 64
    assert list(got) == list(capi.REPORT_DTYPE.names)
    for name in capi.REPORT_DTYPE.names:
        assert capi.REPORT_DTYPE.fields[name][1] == got[name], name

    class Report(C.Structure):
        _fields_ = [(n, {"<i4": C.c_int32, "<i8": C.c_int64, "<f8": C.c_double}[capi.REPORT_DTYPE.fields[n][0].str]) for n in capi.REPORT_DTYPE.names]

    assert C.sizeof(Report) == 64 and all(getattr(Report, n).offset == got[n] for n in got)
    assert capi.load().sdr_abi_version() == 2 and C.sizeof(capi.Results) == 128
    for name in ("sdr_enable_reports", "sdr_reports_enabled", "sdr_poll_reports", "sdr_group_enable_reports", "sdr_group_poll_reports"):
        assert name in capi.SYMBOLS and hasattr(capi.load(), name)
    assert capi.KERNELS == ("k_fft_psd", "k_window_means", "k_noise_stats", "k_thresholds", "k_listen_gather", "k_cumulate",
                            "k_find_peaks", "k_listen_decode")
