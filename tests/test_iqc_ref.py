"""The IQ correction without a GPU (include/sdrainer_hip.h "IQ correction"; tests/iqc_ref.py is its NumPy restatement):
sdr_iq_correction_from_sums gives the bits of the float64 sequence for random and extreme sums of each format, and every
refusal leaves its output untouched; the host code of the sums (csrc/host/iq_sums.h: units, the bookkeeping of n and skipped
around 2^32) is walked by a stand-alone program, built plain and under the address and undefined-behaviour sanitizers; and
the impaired end-to-end fixture is held to the oracle receiver alone: uncorrected it shows a ghost of either station and the
DC line, and the ghost decodes to the call sign; corrected from the stream's own sums they are gone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ddc_ref as R
import iqc_ref as Q
from parity_tools import capi  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SRC = os.path.join(ROOT, "tests", "host", "test_iq_sums_host.cpp")
MARK = (1.5, 2.5, 3.5, 4.5)


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


def library_from_sums(capi, s, fmt):
    """(status, the four float32 values as uint32 words) with the output preset to MARK."""
    out = capi.IqCorrection(*MARK)
    sums = capi.IqSums(**s)
    rc = capi.load().sdr_iq_correction_from_sums(C.byref(sums), fmt, C.byref(out))
    return rc, np.array(out.astuple(), np.float32).view(np.uint32)


def impaired_raw(fmt, n, seed):
    """Noise with a DC offset and an imbalance drawn from the seed, quantised to the format."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, rng.uniform(0.02, 0.25), (n, 2))
    y = Q.synth.impair_iq(x, rng.uniform(0.8, 1.25), rng.uniform(-0.2, 0.2), rng.uniform(-0.1, 0.1, 2))
    return Q.synth.quantise_iq(y, Q.SUM_FORMAT_IDS[Q.SUM_FORMATS.index(fmt)])


def check_equal(capi, s, fmt):
    want = Q.from_sums(s, fmt)
    rc, got = library_from_sums(capi, s, fmt)
    if want is None:
        assert rc == capi.ERR_BAD_ARG and np.array_equal(got, np.array(MARK, np.float32).view(np.uint32)), (s, fmt)
    else:
        assert rc == capi.OK and np.array_equal(got, np.array(want, np.float32).view(np.uint32)), (s, fmt, want)
    return want


@pytest.mark.parametrize("fmt", Q.SUM_FORMATS, ids=Q.SUM_FORMAT_IDS)
def test_from_sums_gives_the_bits_of_the_float64_sequence(capi, fmt):
    accepted = 0
    for seed in range(40):
        n = int(np.random.default_rng(seed).integers(2, 5000))
        s = Q.sums(impaired_raw(fmt, n, 1000 * fmt + seed), fmt)
        accepted += check_equal(capi, s, fmt) is not None
        # the same stream repeated until it holds 2^32 samples or nearly: every sum times k
        k = (1 << 32) // n
        accepted += check_equal(capi, {f: v * k for f, v in s.items()}, fmt) is not None
    assert accepted >= 70  # (a stream of two or three samples may have no variance)
    # what the estimate is for: the stream's impairment comes out
    raw = impaired_raw(fmt, 1 << 16, 5)
    corr = Q.from_sums(Q.sums(raw, fmt), fmt)
    y = Q.correct(R.to_f32(raw, fmt), corr).astype(np.float64)
    assert abs(y.mean(0)).max() < 1e-6 and abs(np.mean(y[:, 0] * y[:, 1])) < 1e-6 * y.var()
    assert abs(y[:, 0].var() / y[:, 1].var() - 1) < 1e-5


@pytest.mark.parametrize("fmt", Q.SUM_FORMATS, ids=Q.SUM_FORMAT_IDS)
def test_from_sums_at_the_extremes(capi, fmt):
    lo = int(Q.units(np.array([[np.iinfo(R.RAW_DTYPE[fmt]).min] * 2]), fmt)[0, 0])
    hi = int(Q.units(np.array([[np.iinfo(R.RAW_DTYPE[fmt]).max] * 2]), fmt)[0, 0])
    n = 1 << 32
    # every sample at the most negative word, n = 2^32: no variance, refused, and the largest sums there are
    s = dict(n=n, sum_i=n * lo, sum_q=n * lo, sum_ii=n * lo * lo, sum_qq=n * lo * lo, sum_iq=n * lo * lo, skipped=0, reserved=0)
    assert s["sum_ii"] <= 1 << 62
    assert check_equal(capi, s, fmt) is None
    # I and Q at the extremes, independently: the four corners a quarter each, then with a few samples moved to one corner
    h = n // 4
    for extra in (0, 12345):
        cnt = {(lo, lo): h + extra, (lo, hi): h, (hi, lo): h, (hi, hi): h - extra}
        s = dict(n=n, sum_i=sum(c * i for (i, q), c in cnt.items()), sum_q=sum(c * q for (i, q), c in cnt.items()),
                 sum_ii=sum(c * i * i for (i, q), c in cnt.items()), sum_qq=sum(c * q * q for (i, q), c in cnt.items()),
                 sum_iq=sum(c * i * q for (i, q), c in cnt.items()), skipped=0, reserved=0)
        assert check_equal(capi, s, fmt) is not None


def test_from_sums_refusals_leave_the_output_untouched(capi):
    good = Q.sums(impaired_raw(R.CS8, 1000, 3), R.CS8)
    assert check_equal(capi, good, R.CS8) is not None
    for fmt in (R.F32, 4, -1, 16, 17, 18, 19):
        assert check_equal(capi, good, fmt) is None
    bad = [dict(good, n=1), dict(good, n=0), dict(good, n=-5),
           dict(n=4, sum_i=20, sum_q=0, sum_ii=100, sum_qq=400, sum_iq=0, skipped=0, reserved=0),   # I constant
           dict(n=4, sum_i=0, sum_q=0, sum_ii=20, sum_qq=80, sum_iq=40, skipped=0, reserved=0),     # Q = 2 I
           dict(n=4, sum_i=0, sum_q=0, sum_ii=20, sum_qq=0, sum_iq=0, skipped=0, reserved=0),       # Q constant
           dict(good, sum_ii=-good["sum_ii"])]                                                      # (not sums of anything)
    for s in bad:
        assert check_equal(capi, s, R.CS8) is None
    L = capi.load()
    out = capi.IqCorrection(*MARK)
    assert L.sdr_iq_correction_from_sums(None, R.CS8, C.byref(out)) == capi.ERR_BAD_ARG and out.astuple() == MARK
    assert L.sdr_iq_correction_from_sums(C.byref(capi.IqSums(**good)), R.CS8, None) == capi.ERR_BAD_ARG
    with pytest.raises(capi.SdrError):
        capi.iq_correction_from_sums(dict(good, n=1), R.CS8)
    assert np.array_equal(np.array(capi.iq_correction_from_sums(good, R.CS8).astuple(), np.float32), np.array(Q.from_sums(good, R.CS8)))


@pytest.mark.parametrize("sanitizer", [None, "address,undefined"])
def test_sums_bookkeeping_on_the_host(tmp_path, sanitizer):
    exe = str(tmp_path / "test_iq_sums_host")
    flags = [f"-fsanitize={sanitizer}", "-fno-sanitize-recover=all"] if sanitizer else []
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, HOST_SRC], capture_output=True, text=True)
    if sanitizer and cc.returncode != 0 and "sanitize" in cc.stderr and "error:" not in cc.stderr.replace("-Werror", ""):
        pytest.skip("this compiler has no -fsanitize=" + sanitizer)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.split() == ["iq", "sums", "ok"]
    # the header's from_sums built by another compiler gives NumPy's bits too
    for fmt in Q.SUM_FORMATS:
        s = Q.sums(impaired_raw(fmt, 3000, 77 + fmt), fmt)
        out = subprocess.run([exe, str(fmt)] + [str(s[f]) for f in Q.FIELDS[:6]], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        assert [int(w, 16) for w in out.stdout.split()] == [int(v) for v in np.array(Q.from_sums(s, fmt), np.float32).view(np.uint32)]


def test_the_stateful_reference_is_the_plain_one_for_a_constant_correction(table):
    d, t, steps = 3, 7, (100, -200)
    taps = np.random.default_rng(1).uniform(-1, 1, t).astype(np.float32)
    raw = R.random_raw(d * 40, R.CS8, 2)
    x = R.to_f32(raw, R.CS8)
    corr = (0.01, -0.02, 1.05, -0.03)
    want = R.ddc_ref(Q.correct(x, corr), d, taps, steps, *table)
    ref = Q.CorrectedDdcRef(d, taps, steps, *table)
    got = np.concatenate([ref.process(x[a:e], corr) for a, e in ((0, d), (d, 3 * d), (3 * d, 20 * d), (20 * d, 40 * d))], axis=1)
    assert got.tobytes() == want.tobytes()
    # removed: the bits of the uncorrected reference from T - 1 samples behind the change on, and other bits in front
    ref = Q.CorrectedDdcRef(d, taps, steps, *table)
    got = np.concatenate([ref.process(x[:20 * d], corr), ref.process(x[20 * d:], None)], axis=1)
    plain = R.ddc_ref(x, d, taps, steps, *table)
    assert got[:, 20:].tobytes() == plain[:, 20:].tobytes() and got[:, :20].tobytes() == want[:, :20].tobytes()
    assert got[:, :20].tobytes() != plain[:, :20].tobytes()


def test_impaired_fixture_shows_ghosts_and_the_correction_removes_them(table):
    e = Q.E2E
    plain = Q.e2e_reference(table, corrected=False)
    raw = plain["raw"]
    assert raw.dtype == np.uint8 and raw.min() > 0 and raw.max() < 255  # (nothing clipped)
    ghost_listener = (1, 1)  # band 1's listener on bin 192: the image of band 0's "dl1abc"
    assert Q.LISTEN[1][1] == Q.GHOST_BINS[1]
    for b, g in enumerate(Q.GHOST_BINS):
        assert Q.peaks_near(plain["outs"][b], g, 1) >= 1, f"uncorrected: no peak at the ghost bin {g} of band {b}"
    assert e["calls"][0] in plain["decs"][ghost_listener[0]][ghost_listener[1]][0], "uncorrected: the ghost does not decode"
    fixed = Q.e2e_reference(table, corrected=True)
    assert fixed["corr"] is not None
    dc_re, dc_im, gain_im, cross = (float(v) for v in fixed["corr"])
    assert abs(dc_re - e["dc"][0]) < 2e-3 and abs(dc_im - e["dc"][1]) < 2e-3
    assert abs(gain_im - 1 / (e["gain"] * np.cos(e["phase"]))) < 5e-3 and abs(cross + np.tan(e["phase"])) < 5e-3
    for b in range(3):
        for g in Q.GHOST_BINS:
            assert Q.peaks_near(fixed["outs"][b], g, 2) == 0, f"corrected: a peak near bin {g} of band {b}"
    assert e["calls"][0] not in fixed["decs"][ghost_listener[0]][ghost_listener[1]][0], "corrected: the ghost still decodes"
    for which in (plain, fixed):
        for b, call in enumerate(e["calls"]):
            assert call in which["decs"][b][0][0], which["decs"][b][0][0]
            assert Q.peaks_near(which["outs"][b], e["bins"][b], 0) >= 3  # (cumulations that hold the carrier)
