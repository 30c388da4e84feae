"""The fine converter's contract on the CPU (no GPU): the binding's constants, the NumPy restatement tests/fine_ref.py that the
GPU tests compare with - against tests/ddc_ref.py band by band, under cuts of the streams and under changes of the map -
sdr_fine_tune against its integer definition, a tone through channelizer and fine converter, and the end-to-end fixture
through the oracle receiver, so that the GPU test's input is one on which the reference chain itself succeeds."""
import ctypes
import os
import re

import numpy as np
import pytest

import chan_ref as CR
import ddc_ref as R
import fine_ref as F
from parity_tools import bits_equal, capi, run_oracle  # noqa: F401

L = R.L
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


def streams(n_inputs, n, seed):
    return np.stack([R.random_raw(n, R.F32, seed + i) for i in range(n_inputs)])


def test_capi_constants_match_the_header(capi):
    header = open(os.path.join(ROOT, "include", "sdrainer_hip.h")).read()
    assert ctypes.sizeof(capi.FineConfig) == 32
    body = re.search(r"typedef struct sdr_fine_config \{(.*?)\} sdr_fine_config;", header, re.S).group(1)
    assert re.findall(r"int32_t (\w+);", body) == [f for f, _ in capi.FineConfig._fields_]
    assert all(t is ctypes.c_int32 for _, t in capi.FineConfig._fields_)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sdr_fine_\w+)\s*\(", code)))
    assert len(declared) == 10 and all(n in capi.SYMBOLS for n in declared)
    assert capi.load().sdr_abi_version() == 2
    # the sets of the other front-end calls stay what they were, and no name ends in iq8 that did not
    for prefix, count in (("sdr_ddc_", 10), ("sdr_chan_", 9), ("sdr_iq_", 7), ("sdr_nb_", 12)):
        assert len(set(re.findall(r"\b(" + prefix + r"\w+)\s*\(", code))) == count, prefix
    assert not [n for n in declared if n.endswith("iq8")]


def test_a_fixed_map_equals_the_ddc_reference_per_band(table):
    d, t = 6, 48
    steps, inputs = (0, 9000, -32768, -1), (2, 0, 2, 0)
    taps = np.random.default_rng(3).uniform(-1, 1, t).astype(np.float32)
    x = streams(3, d * 300, 10)
    got = F.fine_ref(x, d, taps, steps, *table, inputs=inputs)
    for b, (s, i) in enumerate(zip(steps, inputs)):
        assert bits_equal(got[b], R.ddc_ref(x[i], d, taps, (s,), *table)[0]), b
    # the default map: band b reads input b
    assert bits_equal(F.fine_ref(x, d, taps, steps[:3], *table)[1], R.ddc_ref(x[1], d, taps, (9000,), *table)[0])
    # and the index is the streams' own
    k0 = d * 54321
    moved = F.fine_ref(x, d, taps, steps, *table, inputs=inputs, first_sample=k0)
    assert bits_equal(moved[1], R.ddc_ref(x[0], d, taps, (9000,), *table, first_sample=k0)[0]) and not bits_equal(moved[1], got[1])


def test_cutting_the_streams_changes_no_bit(table):
    d, t = 6, 48
    steps, inputs = (9000, -7, 0), (1, 1, 0)
    taps = R.synth.lowpass_taps(d, 8)
    x = streams(2, d * 400, 20)
    whole = F.fine_ref(x, d, taps, steps, *table, inputs=inputs)
    cut = F.FineRef(2, d, taps, steps, *table, inputs=inputs)
    lens = (d, 5 * d, 3 * d, 3 * d, 100 * d)  # calls of one output, and two in a row shorter than T - 1
    assert 3 * d < t - 1
    lens += (x.shape[1] - sum(lens),)
    pieces, a = [], 0
    for n in lens:
        pieces.append(cut.process(x[:, a:a + n]))
        a += n
    assert a == x.shape[1] and cut.total == a and bits_equal(np.concatenate(pieces, axis=1), whole)


def test_a_change_of_the_map_holds_from_the_next_call(table):
    """A band moved to an input nobody read so far finds that input's history: its outputs behind the move equal a DDC that
    read the input from the start with the step that is current."""
    d, t = 4, 32
    taps = np.random.default_rng(4).uniform(-1, 1, t).astype(np.float32)
    x = streams(3, d * 120, 30)
    ref = F.FineRef(3, d, taps, (100, -200), *table, inputs=(0, 2))
    a = ref.process(x[:, :d * 40])
    ref.set_input(0, 1)
    ref.set_nco_step(1, 77)
    b = ref.process(x[:, d * 40:d * 43])
    ref.set_input(0, 0)
    c = ref.process(x[:, d * 43:])
    got = np.concatenate([a, b, c], axis=1)
    on0, on1 = R.ddc_ref(x[0], d, taps, (100,), *table)[0], R.ddc_ref(x[1], d, taps, (100,), *table)[0]
    assert bits_equal(got[0, :40], on0[:40]) and bits_equal(got[0, 40:43], on1[40:43]) and bits_equal(got[0, 43:], on0[43:])
    assert bits_equal(got[1, :40], R.ddc_ref(x[2], d, taps, (-200,), *table)[0][:40])
    assert bits_equal(got[1, 40:], R.ddc_ref(x[2], d, taps, (77,), *table)[0][40:])


# -- sdr_fine_tune ---------------------------------------------------------------------------------------------------------
def test_fine_tune_values(capi):
    assert capi.fine_tune(8, 4, 37568) == (1, 4800)
    assert capi.fine_tune(8, 4, -2 * 32768 - 6400) == (6, -6400)  # channel -2 of 8
    assert capi.fine_tune(8, 4, -1) == (0, -1) and capi.fine_tune(8, 4, -32768) == (7, 0)
    assert capi.fine_tune(8, 4, 0) == (0, 0)
    # the wide stream's two edges are one channel: M/2
    assert capi.fine_tune(8, 4, 32768 * 4) == (4, 0) and capi.fine_tune(8, 4, -32768 * 4) == (4, 0)
    # a tie goes to the even channel (q = 32768: half way is 16384)
    assert capi.fine_tune(8, 4, 16384) == (0, 16384) and capi.fine_tune(8, 4, 32768 + 16384) == (2, -16384)
    assert capi.fine_tune(8, 4, -16384) == (0, -16384) and capi.fine_tune(8, 4, -32768 - 16384) == (6, 16384)
    # D = M: q = 65536, a step of 32768 does not exist and wraps to the next channel
    assert capi.fine_tune(8, 8, 32768) == (1, -32768) and capi.fine_tune(8, 8, 65536 + 32768) == (2, -32768)
    assert capi.fine_tune(8, 8, -32768) == (0, -32768) and capi.fine_tune(8, 8, 32767) == (0, 32767)
    assert capi.fine_tune(8, 8, 4 * 65536) == (4, 0) and capi.fine_tune(8, 8, 4 * 65536 - 32768) == (4, -32768)
    assert capi.fine_tune(256, 64, 12345) == (1, 12345 - 16384) and capi.fine_tune(2, 1, -30000) == (1, -30000 + 32768)


def test_fine_tune_refusals_leave_the_outputs_alone(capi):
    lib = capi.load()
    ch, st = ctypes.c_int32(-7), ctypes.c_int32(-9)
    bad = [(0, 1, 0), (1, 1, 0), (3, 3, 0), (6, 3, 0), (512, 128, 0), (8, 1, 0), (8, 3, 0), (8, 16, 0), (8, 0, 0), (2, 0, 0), (8, -4, 0),
           (8, 4, 32768 * 4 + 1), (8, 4, -32768 * 4 - 1), (8, 8, 2 ** 40), (8, 8, -2 ** 62)]
    for m, d, target in bad:
        assert lib.sdr_fine_tune(m, d, target, ctypes.byref(ch), ctypes.byref(st)) == capi.ERR_BAD_ARG, (m, d, target)
        assert (ch.value, st.value) == (-7, -9) and lib.sdr_last_error()
        with pytest.raises(capi.SdrError):
            capi.fine_tune(m, d, target)
    assert lib.sdr_fine_tune(8, 4, 0, None, ctypes.byref(st)) == capi.ERR_BAD_ARG
    assert lib.sdr_fine_tune(8, 4, 0, ctypes.byref(ch), None) == capi.ERR_BAD_ARG
    assert (ch.value, st.value) == (-7, -9)
    assert lib.sdr_fine_tune(8, 4, 5, ctypes.byref(ch), ctypes.byref(st)) == capi.OK and (ch.value, st.value) == (0, 5)


def test_fine_tune_identity_by_brute_force(capi):
    rng = np.random.default_rng(5)
    n = 0
    for m, d in ((2, 1), (2, 2), (4, 1), (8, 2), (8, 4), (8, 8), (64, 32), (64, 16), (256, 256), (256, 64)):
        q = L * d // m
        edge = 32768 * d
        targets = set(int(v) for v in rng.integers(-edge, edge + 1, 400))
        targets |= {-edge, edge, 0, -1, 1, q // 2, -q // 2, q // 2 + 1, q // 2 - 1, 3 * q // 2, -3 * q // 2} & set(range(-edge, edge + 1))
        for target in sorted(targets):
            c, step = capi.fine_tune(m, d, target)
            assert (c, step) == F.tune_ref(m, d, target), (m, d, target)
            assert 0 <= c < m and -32768 <= step <= 32767 and abs(step) <= q // 2
            assert (c * q + step - target) % (L * d) == 0, (m, d, target)
            n += 1
    assert n > 3000


def test_a_tone_through_channelizer_and_fine_converter_lands_on_its_bin(capi, table):
    """A tone off the channel grid, the band pointed by sdr_fine_tune: checked on a float64 spectrum of the narrow stream."""
    cos, sin = table
    rate, m, d1, d2, n = 1_536_000, 8, 4, 8, 512
    h1, h2 = R.synth.lowpass_taps(d1, 8), R.synth.lowpass_taps(d2, 8)
    narrow_rate = rate / (d1 * d2)
    f = 1500.0
    for target in (37568, -2 * 32768 - 6400):
        centre = target * rate / (L * d1)
        c, step = capi.fine_tune(m, d1, target)
        assert step != 0 and abs(step * (rate / d1) / L) > narrow_rate / 2  # (without its step the tone is outside the band)
        x = R.synth.wide_stream(d1 * d2 * (n + len(h2)) + d1 * len(h1), rate, [(centre + f, 0.5, None)], noise_sigma=1e-4, seed=1)
        x = x[:len(x) - len(x) % (d1 * d2)]
        one = CR.chan_ref(x, m, d1, h1, cos, sin, channels=(c,))
        y = F.fine_ref(one, d2, h2, (step,), cos, sin)[0][-n:]
        spec = np.abs(np.fft.fft(y[:, 0].astype(np.float64) + 1j * y[:, 1]))
        assert int(np.argmax(spec)) == int(round(f / narrow_rate * n)) == 16
        assert spec[16] > 100 * np.delete(spec, 16).max()
        # and the same band without the step does not have it there
        z = F.fine_ref(one, d2, h2, (0,), cos, sin)[0][-n:]
        assert np.abs(np.fft.fft(z[:, 0].astype(np.float64) + 1j * z[:, 1]))[16] < spec[16] / 100


def test_end_to_end_fixture_decodes_on_the_reference_chain(capi, table):
    e = F.E2E
    for target, want in zip(e["targets"], zip(e["channels"], e["fine_steps"])):
        assert capi.fine_tune(e["n_channels"], e["d1"], target) == want
        assert abs(want[1] * (e["wide_rate"] / e["d1"]) / L) > e["rate"] / 2  # the station lies outside the band round the channel centre
    raw, narrow, one, two = F.e2e_reference(*table)
    assert raw.dtype == np.uint8 and raw.min() > 0 and raw.max() < 255  # (nothing clipped)
    assert one.shape == (2, narrow * e["d2"], 2) and two.shape == (2, narrow, 2)
    _, outs, decs = run_oracle(e["rate"], e["n"], e["edge"], [[b] for b in e["bins"]], list(two), [0, 0], e["hop"])
    for b, call in enumerate(e["calls"]):
        assert call in decs[b][0][0], decs[b][0][0]
        assert sum(any(p[6] == e["bins"][b] for p in pk) for pk in outs[b]["peaks"]) >= 3  # (cumulations that hold the carrier)
