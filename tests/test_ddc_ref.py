"""The down-converter's contract on the CPU (no GPU): the NCO table the library hands out, and the NumPy restatement
tests/ddc_ref.py that the GPU tests compare with - against a float64 evaluation, under cuts of the stream, on a tone, and
end to end through the oracle receiver, so that the GPU test's input is one on which the reference path itself succeeds."""
import numpy as np
import pytest

import ddc_ref as R
from parity_tools import bits_equal, capi, run_oracle  # noqa: F401

L = R.L


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


def test_capi_constants_match_the_header(capi):
    import os
    import re

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdrainer_hip.h")).read()
    define = lambda name: int(re.search(r"#define " + name + r" (\d+)\b", header).group(1))
    assert define("SDR_DDC_NCO_SIZE") == capi.DDC_NCO_SIZE == L
    assert define("SDR_DDC_TILE_OUTPUTS") == capi.DDC_TILE_OUTPUTS
    assert [define("SDR_DDC_" + f.upper()) for f in R.FORMAT_IDS] == [capi.DDC_F32, capi.DDC_SC16, capi.DDC_CS8, capi.DDC_CU8] == list(R.FORMATS)
    import ctypes
    assert ctypes.sizeof(capi.DdcConfig) == 32


def test_nco_table_symmetries_are_exact(table):
    cos, sin = table
    assert cos.dtype == np.float32 and cos.shape == (L,) and sin.shape == (L,)
    i = np.arange(L)
    assert bits_equal(sin, cos[(i - L // 4) % L])
    assert bits_equal(cos[1:], cos[L - i[1:]])
    # COS[i] == -COS[L/2 - i]: bit for bit wherever the value is not zero (both zeros of the table are +0)
    j = np.arange(L // 2 + 1)
    assert np.array_equal(cos[j], -cos[L // 2 - j])
    nz = cos[j] != 0
    assert bits_equal(cos[j][nz], (-cos[L // 2 - j])[nz])
    assert [float(cos[q * L // 4]) for q in range(4)] == [1.0, 0.0, -1.0, 0.0]
    assert [float(sin[q * L // 4]) for q in range(4)] == [0.0, 1.0, 0.0, -1.0]
    assert np.count_nonzero(cos == 0) == 2 and not np.signbit(cos[cos == 0]).any()


def test_nco_table_is_within_one_ulp(table):
    cos, sin = table
    ph = 2.0 * np.pi * np.arange(L, dtype=np.float64) / L
    for got, want in ((cos, np.cos(ph)), (sin, np.sin(ph))):
        exact_zero = np.arange(L) % (L // 4) == 0  # (float64 cos(pi / 2) is 6e-17; the table's 0 is the true value)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err[~exact_zero] <= ulp[~exact_zero]), float((err / ulp)[~exact_zero].max())


@pytest.mark.parametrize("fmt", R.FORMATS, ids=R.FORMAT_IDS)
def test_reference_against_float64(table, fmt):
    cos, sin = table
    d, t, steps = 6, 48, (0, 9000, -32768, -1)
    taps = np.random.default_rng(3).uniform(-1, 1, t).astype(np.float32)
    x = R.to_f32(R.random_raw(d * 700, fmt, 40 + fmt), fmt)
    got = R.ddc_ref(x, d, taps, steps, cos, sin)
    want, ymax = R.ddc_f64(x, d, taps, steps, cos, sin)
    # each y carries three roundings of which the two products' sum to at most 2^-24 max|y|, the sum's a third, bounded
    # together by 2 u max|y|; T products and T sums in order add T u sum|h| max|y| to first order: (T + 2) u sum|h| max|y|
    bound = (t + 2) * 2.0 ** -24 * float(np.abs(taps.astype(np.float64)).sum()) * ymax
    err = float(np.abs(got.astype(np.float64) - want).max())
    assert err <= bound, (err, bound)
    assert err > 0  # (the comparison is not vacuous: float32 sums do round)


def test_cutting_the_stream_changes_no_bit(table):
    cos, sin = table
    d, t, steps = 6, 48, (9000, -7, 0)
    taps = R.synth.lowpass_taps(d, 8)
    x = R.to_f32(R.random_raw(d * 400, R.SC16, 8), R.SC16)
    whole = R.ddc_ref(x, d, taps, steps, cos, sin)
    cut = R.DdcRef(d, taps, steps, cos, sin)
    pieces, a = [], 0
    for n in (d, 5 * d, 100 * d, len(x) - 106 * d):
        pieces.append(cut.process(x[a:a + n]))
        a += n
    assert a == len(x) and bits_equal(np.concatenate(pieces, axis=1), whole)
    # and with the stream's index moved: the phase follows the absolute index
    moved = R.ddc_ref(x, d, taps, steps, cos, sin, first_sample=6 * 12345)
    assert bits_equal(moved[2], whole[2]) and not bits_equal(moved[0], whole[0])


def test_a_tone_lands_on_its_bin(table):
    cos, sin = table
    rate, d, step, f, n = 288_000, 6, 9000, 1500.0, 512
    taps = R.synth.lowpass_taps(d, 8)
    x = R.synth.wide_stream(d * (n + len(taps)), rate, [(step * rate / L + f, 0.5, None)], noise_sigma=1e-4, seed=1)
    y = R.ddc_ref(x, d, taps, (step,), cos, sin)[0][-n:]
    spec = np.abs(np.fft.fft(y[:, 0].astype(np.float64) + 1j * y[:, 1]))
    assert int(np.argmax(spec)) == int(round(f / (rate / d) * n)) == 16
    assert spec[16] > 100 * np.delete(spec, 16).max()


def test_end_to_end_fixture_decodes_on_the_reference_path(table):
    cos, sin = table
    e = R.E2E
    raw, narrow = R.e2e_wide()
    assert raw.dtype == np.uint8 and raw.min() > 0 and raw.max() < 255  # (nothing clipped)
    out = R.ddc_ref(R.to_f32(raw, R.CU8), e["decimation"], R.e2e_taps(), e["steps"], cos, sin)
    assert out.shape == (2, narrow, 2)
    _, outs, decs = run_oracle(e["rate"], e["n"], e["edge"], [[b] for b in e["bins"]], list(out), [0, 0], e["hop"])
    for b, call in enumerate(e["calls"]):
        assert call in decs[b][0][0], decs[b][0][0]
        assert sum(any(p[6] == e["bins"][b] for p in pk) for pk in outs[b]["peaks"]) >= 3  # (cumulations that hold the carrier)
