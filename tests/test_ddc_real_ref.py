"""The down-converter's real input formats on the CPU (no GPU): the constants of header, binding and helper, and the
reference path on a real stream - tests/ddc_ref.py fed (v, +0.0) - against float64, on a real tone (its bin with +step, the
mirrored bin with -step, half the amplitude) and end to end through the oracle receiver, so that the GPU test's input is
one on which the reference path itself succeeds."""
import ctypes
import os
import re

import numpy as np
import pytest

import ddc_real as DR
import ddc_ref as R
from parity_tools import capi, run_oracle  # noqa: F401

L = R.L


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


def test_capi_constants_match_the_header(capi):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdrainer_hip.h")).read()
    define = lambda name: int(re.search(r"#define " + name + r" +(\d+)\b", header).group(1))
    assert define("SDR_DDC_REAL") == capi.DDC_REAL == DR.REAL == 16
    names = ("RF32", "RS16", "RS8", "RU8")
    assert [define("SDR_DDC_" + n) for n in names] == [getattr(capi, "DDC_" + n) for n in names] == list(DR.FORMATS) == [16, 17, 18, 19]
    assert [capi.DDC_REAL | f for f in (capi.DDC_F32, capi.DDC_SC16, capi.DDC_CS8, capi.DDC_CU8)] == list(DR.FORMATS)
    assert [np.dtype(DR.RAW_DTYPE[f]).itemsize for f in DR.FORMATS] == [4, 2, 1, 1]
    assert ctypes.sizeof(capi.DdcConfig) == 32


def test_raw_values_are_the_complex_formats(capi):
    """A raw word's value is its complex format's, and random_raw_real covers what it says."""
    assert DR.to_f32_real(np.array([-32768, -1, 0, 32767]), DR.RS16).tolist() == [np.float32(-32768) / np.float32(32767), np.float32(-1) / np.float32(32767), 0.0, 1.0]
    assert DR.to_f32_real(np.array([-128, 0, 127]), DR.RS8).tolist() == [-1.0, 0.0, 127 / 128]
    assert DR.to_f32_real(np.array([0, 127, 128, 255]), DR.RU8).tolist() == [-255 / 256, -1 / 256, 1 / 256, 255 / 256]
    for fmt in (DR.RS8, DR.RU8):
        assert len(np.unique(DR.random_raw_real(256, fmt, 1))) == 256
    r = DR.random_raw_real(5, DR.RS16, 2)
    assert r.dtype == np.int16 and r.min() == -32768 and r.max() == 32767
    z = DR.as_complex(np.array([-0.0, 1.0], np.float32))
    assert z.dtype == np.float32 and z.shape == (2, 2) and not np.signbit(z[:, 1]).any() and np.signbit(z[0, 0])


@pytest.mark.parametrize("fmt", DR.FORMATS, ids=DR.FORMAT_IDS)
def test_reference_against_float64(table, fmt):
    cos, sin = table
    d, t, steps = 6, 48, (0, 9000, -32768, -1)
    taps = np.random.default_rng(3).uniform(-1, 1, t).astype(np.float32)
    x = DR.as_complex(DR.to_f32_real(DR.random_raw_real(d * 700, fmt, 60 + fmt), fmt))
    got = R.ddc_ref(x, d, taps, steps, cos, sin)
    want, ymax = R.ddc_f64(x, d, taps, steps, cos, sin)
    # the bound tests/test_ddc_ref.py derives: (T + 2) u sum|h| max|y| (with im = 0 a y carries fewer roundings, not more)
    bound = (t + 2) * 2.0 ** -24 * float(np.abs(taps.astype(np.float64)).sum()) * ymax
    err = float(np.abs(got.astype(np.float64) - want).max())
    assert 0 < err <= bound, (err, bound)


@pytest.mark.parametrize("sign", [1, -1], ids=["+step", "-step"])
def test_a_real_tone_lands_on_its_bin_at_half_amplitude(table, sign):
    cos, sin = table
    rate, d, step, f, n, a = 288_000, 6, 9000, 1500.0, 512, 0.5
    taps = R.synth.lowpass_taps(d, 8)
    v = R.synth.wide_stream_real(d * (n + len(taps)), rate, [(step * rate / L + f, a, None)], noise_sigma=1e-4, seed=1)
    assert v.dtype == np.float32 and v.shape == (d * (n + len(taps)),)
    y = R.ddc_ref(DR.as_complex(v), d, taps, (sign * step,), cos, sin)[0][-n:]
    spec = np.abs(np.fft.fft(y[:, 0].astype(np.float64) + 1j * y[:, 1]))
    at = 16 if sign > 0 else n - 16  # the mirror image: the band's spectrum reversed
    assert int(round(f / (rate / d) * n)) == 16 and int(np.argmax(spec)) == at
    assert spec[at] > 100 * np.delete(spec, at).max()
    # A cos(..) = A/2 e^(+i..) + A/2 e^(-i..): one half reaches the band (the taps sum to 1 and are flat at 1500 Hz to well
    # under the percent)
    assert abs(spec[at] / n - a / 2) <= 0.01 * a / 2, spec[at] / n


@pytest.mark.parametrize("quantise", sorted(DR.QUANTISED))
def test_end_to_end_fixture_decodes_on_the_reference_path(table, quantise):
    cos, sin = table
    e = DR.E2E_REAL
    raw, narrow = DR.e2e_real_wide(quantise)
    fmt = DR.QUANTISED[quantise]
    info = np.iinfo(DR.RAW_DTYPE[fmt])
    assert raw.dtype == DR.RAW_DTYPE[fmt] and raw.shape == (narrow * e["decimation"],)
    assert raw.min() > info.min and raw.max() < info.max  # (nothing clipped)
    out = R.ddc_ref(DR.as_complex(DR.to_f32_real(raw, fmt)), e["decimation"], DR.e2e_real_taps(), e["steps"], cos, sin)
    assert out.shape == (3, narrow, 2)
    _, outs, decs = run_oracle(e["rate"], e["n"], e["edge"], [[b] for b in e["bins"]], list(out), [0, 0, 0], e["hop"])
    for b, call in enumerate(e["calls"]):
        assert call in decs[b][0][0], decs[b][0][0]
        assert sum(any(p[6] == e["bins"][b] for p in pk) for pk in outs[b]["peaks"]) >= 3  # (cumulations that hold the carrier)
