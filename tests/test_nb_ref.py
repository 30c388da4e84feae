"""The impulse noise blanker without a GPU: sdr_nb_blank_host (plain C++ integers, csrc/host/nb_rule.h) against
tests/nb_ref.py byte for byte, statistics included - every format, block and window sizes from the smallest to
B * W = 65536, holds 0 .. B, ratios from "off" to the largest, random words with full-scale samples planted where a block, a
16-byte group or the stream ends; the reference fed in pieces against the reference fed whole; the extreme values that
bound the 64-bit inequality; and what the definition does to Gaussian noise with planted pulses, on the raw stream and
behind tests/ddc_ref.py."""
import numpy as np
import pytest

import ddc_ref as R
import nb_ref as N


@pytest.fixture(scope="module")
def capi():
    from sdrainer_amd.csrc import build
    build.build()
    from sdrainer_amd import capi as c
    return c


GEOMETRIES = [(64, 1), (64, 2), (256, 8), (4096, 16)]
RATIOS = (0, 16, 192, 16384)


def planted(fmt, b, w, seed, quiet):
    """(raw, places): random words - over the whole range, or a few LSB around the centre so that the largest ratio is
    reached - with full-scale samples at a block's first and last sample, the last sample of a 16-byte group, two places
    closer than a hold of 3, and the stream's last sample; all in judged blocks."""
    blocks = w + 6
    n = blocks * b
    spread = None if not quiet else (100 if (fmt & ~N.REAL) == N.SC16 else 3)
    raw = N.random_raw(n, fmt, seed, spread)
    per_group = 16 // raw[:1].nbytes
    j = w + 1
    places = [j * b, (j + 1) * b - 1, (j + 2) * b + per_group - 1, (j + 3) * b + 20, (j + 3) * b + 22, n - 1]
    for p in places:
        raw[p] = N.full_scale(fmt)
    return raw, places


@pytest.mark.parametrize("fmt", N.FORMATS, ids=N.FORMAT_IDS)
@pytest.mark.parametrize("b,w", GEOMETRIES)
def test_blank_host_equals_the_reference(capi, fmt, b, w):
    seen = 0
    for quiet in (True, False):
        raw, places = planted(fmt, b, w, 1000 * b + 10 * w + fmt, quiet)
        for hold in (0, 1, 3, b):
            for ratio in RATIOS:
                want, wstats = N.nb_ref(raw, fmt, b, w, ratio, hold)
                got, gstats = capi.nb_blank_host(raw, fmt, b, w, ratio, hold)
                assert got.dtype == want.dtype and got.shape == want.shape
                assert np.array_equal(got, want), (quiet, hold, ratio)
                assert gstats == wstats, (quiet, hold, ratio)
                assert wstats["samples"] == len(raw) and (ratio != 0 or wstats["blanked"] == 0)
                if quiet and ratio != 0:
                    # the first planted sample has a clean window behind it: an impulse at every ratio (the later ones
                    # are judged against a level that holds the earlier ones' power)
                    assert wstats["impulses"] >= 1 and not np.array_equal(want[places[0]], raw[places[0]])
                    assert wstats["blanked"] >= min(hold + 1, len(raw) - places[0])
                    seen += 1
                assert np.array_equal(want[:w * b], raw[:w * b])  # the first W blocks are never judged
    assert seen == 12


@pytest.mark.parametrize("fmt", N.FORMATS, ids=N.FORMAT_IDS)
def test_reference_in_pieces_equals_the_reference_whole(fmt):
    b, w = 64, 8
    raw, _ = planted(fmt, b, w, 31 + fmt, True)
    raw[5 * b - 1] = N.full_scale(fmt)  # (unjudged)
    raw[(w + 2) * b - 1] = N.full_scale(fmt)  # a gate across a cut
    for hold in (0, 3, b):
        want, wstats = N.nb_ref(raw, fmt, b, w, 64, hold)
        ref = N.NbRef(fmt, b, w, 64, hold)
        lens = [b, 5 * b, b, b, 2 * b, b]
        lens.append(len(raw) - sum(lens))
        cuts = np.cumsum([0] + lens)
        got = np.concatenate([ref.process(raw[a:e]) for a, e in zip(cuts[:-1], cuts[1:])])
        assert np.array_equal(got, want) and ref.read_stats() == wstats
        assert wstats["blanked"] > wstats["impulses"] or hold == 0


def test_the_extreme_values_do_not_wrap_64_bits(capi):
    """sc16 (-32768, -32768) everywhere, B * W = 65536, ratio_q4 = 16384: the two sides of the inequality at their largest."""
    b, w = 4096, 16
    raw = np.full(((w + 2) * b, 2), -32768, np.int16)
    m = int(N.mags(raw[:1], N.SC16)[0])
    left, right = m * b * w * 16, 16384 * (m * b * w)
    assert m == 2 ** 31 and left == 2 ** 51 < 2 ** 52 and right == 2 ** 61 < 2 ** 62 < 2 ** 64
    for ratio, impulses in ((16384, 0), (17, 0), (16, 0)):  # 16: both sides equal, and "greater" decides
        got, stats = capi.nb_blank_host(raw, N.SC16, b, w, ratio, 3)
        assert stats == N.nb_ref(raw, N.SC16, b, w, ratio, 3)[1] and stats["impulses"] == impulses
        assert np.array_equal(got, raw)
    # a quiet window in front of one extreme sample: the largest left side against a small right side
    raw[:w * b] = 1
    raw[w * b + 1:] = 1
    got, stats = capi.nb_blank_host(raw, N.SC16, b, w, 16384, 0)
    want, wstats = N.nb_ref(raw, N.SC16, b, w, 16384, 0)
    assert np.array_equal(got, want) and stats == wstats and stats["impulses"] == 1 and not got[w * b].any()


# -- behaviour ----------------------------------------------------------------------------------------------------------------
NOISE = dict(b=256, w=8, hold=3, ratio=192, sigma=20.0, n=64 * 256, pulses=40, seed=5)


def noise_with_pulses():
    """cu8 Gaussian noise of sigma = 20 LSB around 127.5 with 40 samples (255, 0) planted in judged blocks, 200 apart."""
    c = NOISE
    rng = np.random.default_rng(c["seed"])
    raw = np.clip(np.rint(127.5 + c["sigma"] * rng.standard_normal((c["n"], 2))), 0, 255).astype(np.uint8)
    places = c["w"] * c["b"] + 5 + 200 * np.arange(c["pulses"])
    assert places[-1] + c["hold"] < c["n"]
    raw[places] = (255, 0)
    return raw, places


def test_planted_pulses_are_blanked_and_nothing_else():
    c = NOISE
    raw, places = noise_with_pulses()
    ref = N.NbRef(N.CU8, c["b"], c["w"], c["ratio"], c["hold"])
    out = ref.process(raw)
    stats = ref.read_stats()
    changed = np.flatnonzero((out != raw).any(axis=1))
    gates = (places[:, None] + np.arange(c["hold"] + 1)[None, :]).reshape(-1)
    print("impulses", stats["impulses"], "blanked", stats["blanked"], "outside the gates", len(np.setdiff1d(changed, gates)))
    m = N.mags(raw, N.CU8)
    for p in places:  # every planted sample is an impulse by the definition, evaluated here in Python integers
        j = p // c["b"]
        level = int(m[(j - c["w"]) * c["b"]:j * c["b"]].sum())
        assert int(m[p]) * c["b"] * c["w"] * 16 > c["ratio"] * level
    assert np.isin(places, changed).all()
    assert len(np.setdiff1d(changed, gates)) == 0
    assert stats["impulses"] == c["pulses"] and stats["blanked"] == c["pulses"] * (c["hold"] + 1)
    blank = out[gates]
    assert np.array_equal(blank, N.blank_words(gates, N.CU8)) and abs(int(N.units(blank, N.CU8).sum())) <= 2


def test_the_band_behind_the_ddc_is_quieter_with_the_blanker(capi):
    """Direction only: one band of tests/ddc_ref.py (D = 8, T = 64) over the noise, which holds no signal, with and without
    the blanker in front."""
    c = NOISE
    raw, _ = noise_with_pulses()
    out, _ = N.nb_ref(raw, N.CU8, c["b"], c["w"], c["ratio"], c["hold"])
    table = capi.ddc_nco_table()
    taps = R.e2e_taps()
    assert len(taps) == 64
    power = []
    for stream in (raw, out):
        y = R.ddc_ref(R.to_f32(stream, R.CU8), 8, taps, (9000,), *table)[0, c["w"] * c["b"] // 8:].astype(np.float64)
        power.append(float((y * y).sum(axis=1).mean()))
    print("band power without the blanker %.6e, with it %.6e" % tuple(power))
    assert power[1] < power[0]
