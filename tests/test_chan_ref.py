"""The channelizer's contract on the CPU (no GPU): the binding's constants and struct against the header, and the NumPy
restatement tests/chan_ref.py that the GPU tests compare with - against a float64 evaluation of the equivalent DDC bands,
under cuts of the stream, under a moved first sample, under channel selection, and end to end through the oracle receiver,
so that the GPU test's input is one on which the reference path itself succeeds."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import chan_ref as CR
import ddc_ref as R
from parity_tools import bits_equal, capi, run_oracle  # noqa: F401

L = CR.L
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


def test_capi_constants_and_struct_match_the_header(capi):
    header = open(os.path.join(ROOT, "include", "sdrainer_hip.h")).read()
    body = re.search(r"typedef struct sdr_chan_config \{(.*?)\} sdr_chan_config;", header, re.S).group(1)
    fields = re.findall(r"int32_t (\w+);", body)
    assert fields == [f for f, _ in capi.ChanConfig._fields_]
    assert all(t is ctypes.c_int32 for _, t in capi.ChanConfig._fields_) and ctypes.sizeof(capi.ChanConfig) == 32
    assert [f for f, _ in capi.ChanConfig._fields_[:1] + capi.ChanConfig._fields_[2:7]] == [f for f, _ in capi.DdcConfig._fields_[:1] + capi.DdcConfig._fields_[2:7]]
    define = lambda name: int(re.search(r"#define " + name + r" (\d+)\b", header).group(1))
    assert define("SDR_DDC_NCO_SIZE") == L
    assert CR.FORMATS == (capi.DDC_F32, capi.DDC_SC16, capi.DDC_CS8, capi.DDC_CU8, capi.DDC_RF32, capi.DDC_RS16, capi.DDC_RS8, capi.DDC_RU8)
    for name in ("create", "destroy", "sync", "set_stream", "set_first_sample", "total_samples", "process_device", "process_host", "tile_outputs"):
        assert "sdr_chan_" + name in capi.SYMBOLS and re.search(r"\bsdr_chan_" + name + r"\(", header)


def test_tile_outputs_accepts_exactly_the_legal_geometries(capi):
    for m in range(0, 600):
        for d in (0, 1, 2, 3, m // 8, m // 4, m // 2, m, 2 * m):
            for t in (0, m, 3 * m, 64 * m, 65 * m, m + 1, 4096, 8192):
                legal = (m in (2, 4, 8, 16, 32, 64, 128, 256) and d >= 1 and d in (m, m // 2, m // 4) and m % d == 0
                         and t >= m and t % m == 0 and t // m <= 64 and t <= 4096)
                tile = capi.chan_tile_outputs(m, d, t)
                assert (tile >= 16) if legal else (tile < 0), (m, d, t, tile)


@pytest.mark.parametrize("fmt", CR.FORMATS, ids=CR.FORMAT_IDS)
@pytest.mark.parametrize("m,d,p", [(8, 8, 4), (8, 4, 4), (16, 4, 3), (64, 32, 8), (2, 1, 5)])
def test_reference_against_float64(table, fmt, m, d, p):
    """Channel c against the DDC band with step c L / M, the same D and taps, evaluated in float64 (ddc_ref.ddc_f64).
    The bound, with u = 2^-24, S = sum |h| and X = max |x| (= the DDC's max |y|: the float64 mix does not change a
    modulus beyond the table's rounding): a branch sum is P products and P sums in order, P u of its own sum |h_r| X to
    first order, and the M branch sums add up to at most P u S X at an output, since each tap belongs to one branch.  An FFT
    stage multiplies by a table entry that is off by at most u / 2, rounds two products and their sum (at most 2 u of the
    product's modulus together, as for the DDC's mix) and rounds the add: at most 4 u of the running modulus, which is
    bounded by S X at every stage because each stage's partial sums are sums over a subset of the taps.  log2 M stages
    give 4 log2 M u S X; 2 u S X is slack for second-order terms.  Together (P + 4 log2 M + 2) u S X."""
    cos, sin = table
    t = p * m
    taps = np.random.default_rng(3 + m).uniform(-1, 1, t).astype(np.float32)
    x = CR.to_f32(CR.random_raw(d * 300, fmt, 40 + fmt), fmt)
    got = CR.chan_ref(x, m, d, taps, cos, sin)
    steps = [CR.channel_step(c, m) for c in range(m)]
    assert steps[m // 2] == -32768 and all(-32768 <= s <= 32767 for s in steps)
    want, ymax = R.ddc_f64(x, d, taps, steps, cos, sin)
    xmax = float(np.abs(x[:, 0].astype(np.float64) + 1j * x[:, 1]).max())
    scale = float(np.abs(taps.astype(np.float64)).sum()) * max(xmax, ymax)
    bound = (p + 4 * math.log2(m) + 2) * 2.0 ** -24 * scale
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"M={m} D={d} P={p} fmt={fmt}: err {err:.3e} = {err / (2.0 ** -24 * scale):.3f} u S X, bound {bound:.3e}")
    assert err <= bound, (err, bound)
    assert err * 4 <= bound, (err, bound)  # (the restatement stays 4x or more under the bound)
    assert err > 0  # (the comparison is not vacuous: float32 sums do round)


def test_cutting_the_stream_changes_no_bit(table):
    cos, sin = table
    m, d, p = 16, 4, 3
    taps = R.synth.lowpass_taps(d, 12)[:m * p]
    assert len(taps) == m * p
    x = R.to_f32(R.random_raw(d * 400, R.SC16, 8), R.SC16)
    whole = CR.chan_ref(x, m, d, taps, cos, sin)
    cut = CR.ChanRef(m, d, taps, cos, sin)
    pieces, a = [], 0
    for n in (d, 5 * d, 2 * d, 3 * d, 100 * d, len(x) - 111 * d):  # (2 D and 3 D: shorter than T - 1, part of the carry survives)
        pieces.append(cut.process(x[a:a + n]))
        a += n
    assert a == len(x) and bits_equal(np.concatenate(pieces, axis=1), whole)


def test_a_moved_first_sample_moves_the_rotation(table):
    """D < M: n D mod M depends on where the stream starts.  A start that is a multiple of M changes nothing; one that is not
    rotates the FFT's input, and the result is still the DDC's bands at the moved index."""
    cos, sin = table
    m, d, p = 16, 4, 3
    taps = np.random.default_rng(5).uniform(-1, 1, m * p).astype(np.float32)
    x = R.to_f32(R.random_raw(d * 200, R.CS8, 9), R.CS8)
    whole = CR.chan_ref(x, m, d, taps, cos, sin)
    assert bits_equal(CR.chan_ref(x, m, d, taps, cos, sin, first_sample=m * 12345), whole)
    k0 = d * 12345
    assert k0 % m != 0
    moved = CR.chan_ref(x, m, d, taps, cos, sin, first_sample=k0)
    assert bits_equal(moved[0], whole[0]) and not bits_equal(moved[1], whole[1])  # (channel 0 has no phase)
    # channel c at the moved index is channel c at index 0 times e^{-j 2 pi c k0 / M}; each side is within the float64 test's
    # bound (P + 4 log2 M + 2) u S X of the exact value, X <= sqrt(2) for cs8
    z = lambda a: a[..., 0].astype(np.float64) + 1j * a[..., 1]
    phase = np.exp(-2j * np.pi * ((np.arange(m) * k0) % m) / m)
    bound = 2 * (p + 4 * 4 + 2) * 2.0 ** -24 * float(np.abs(taps.astype(np.float64)).sum()) * 2 ** 0.5
    err = float(np.abs(z(moved) - z(whole) * phase[:, None]).max())
    assert 0 < err <= bound, (err, bound)
    assert np.abs(z(moved) - z(whole)).max() > 1000 * bound  # (and the phase is no small matter)


def test_channel_selection_equals_rows_of_the_full_output(table):
    cos, sin = table
    m, d, p = 16, 4, 3
    taps = np.random.default_rng(6).uniform(-1, 1, m * p).astype(np.float32)
    x = R.to_f32(R.random_raw(d * 100, R.CU8, 10), R.CU8)
    whole = CR.chan_ref(x, m, d, taps, cos, sin)
    some = CR.chan_ref(x, m, d, taps, cos, sin, channels=(15, 0, 5))
    assert some.shape == (3, 100, 2) and bits_equal(some, whole[[15, 0, 5]])


@pytest.mark.parametrize("m", sorted(CR.SHAPES))
def test_end_to_end_fixture_decodes_on_the_reference_path(table, m):
    cos, sin = table
    e = CR.E2E
    m, d, channels = CR.SHAPES[m]
    assert [CR.channel_step(c, m) for c in channels] == list(e["steps"]) and e["wide_rate"] // d == e["rate"]
    raw, narrow = CR.e2e_wide()
    assert raw.dtype == np.uint8 and raw.min() > 0 and raw.max() < 255  # (nothing clipped)
    out = CR.chan_ref(R.to_f32(raw, R.CU8), m, d, CR.e2e_taps(), cos, sin, channels=channels)
    assert out.shape == (2, narrow, 2)
    _, outs, decs = run_oracle(e["rate"], e["n"], e["edge"], [[b] for b in e["bins"]], list(out), [0, 0], e["hop"])
    for b, call in enumerate(e["calls"]):
        assert call in decs[b][0][0], decs[b][0][0]
        assert sum(any(p[6] == e["bins"][b] for p in pk) for pk in outs[b]["peaks"]) >= 3  # (cumulations that hold the carrier)
