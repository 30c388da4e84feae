"""What keeps tests/test_audio_gpu.py honest, on the CPU: the geometry table is the oracle's, and every case the GPU test
runs is what its name says on the ORACLE's numbers - the streams decode, differ, clip and reach the autoscale cap, the
value regimes put subnormals, huge values, NaN and +0.0 where they say, the ragged writes hold the writes they promise.
These are conditions the generator (tests/audio_gen.py) has to meet, not measurements."""
import numpy as np
import pytest

import audio_gen as gen
from oracle import oracle as orc


def run_oracle(sr, pitch, x, scale, debounce=None):
    ref = orc.AudioDemodulator(pitch, sr)
    ref.set_scale(scale)
    if debounce is not None:
        ref.set_debounce(debounce)
    mags, raw, deb = ref.write(x)
    ref.close()
    return mags, raw, deb, ref.text()


@pytest.mark.parametrize("sr,pitch,bs", gen.GEOMETRY, ids=[f"{g[0]}-{g[1]:g}" for g in gen.GEOMETRY])
def test_geometry_table(sr, pitch, bs):
    assert orc.AudioDemodulator(pitch, sr).blocksize == bs


def test_geometry_table_covers_the_issue():
    assert {g[2] for g in gen.GEOMETRY} >= {0, 39, 48, 60, 80, 200, 207, 288}
    assert set(gen.MANY_GEOMETRY) | {g[:2] for g in gen.SMALL_GEOMETRY} == {g[:2] for g in gen.GEOMETRY if g[2]}


MANY = [c for c in gen.MANY if c[2] >= 64]


@pytest.mark.parametrize("sr,pitch,n,scale", MANY, ids=[f"{c[0]}-{c[2]}-{c[3]:g}" for c in MANY])
def test_many_streams_inputs(sr, pitch, n, scale):
    xs = gen.streams(sr, pitch, n, gen.SEED)
    bs = gen.blocksize(sr, pitch)
    assert len(xs) == n and len({x.size for x in xs}) == 1 and all(x.dtype == np.float32 for x in xs)
    assert xs[0].size // bs > 2 * 1024, "a stream needs several writes of max_blocks = 1024"
    got = [run_oracle(sr, pitch, x, scale)[3] for x in xs]
    want = gen.texts(n)
    exact = sum(g == w for g, w in zip(got, want))
    nonempty = sum(bool(g) for g in got)
    print(f"exact {exact} nonempty {nonempty} distinct {len(set(got))} of {n}")
    assert 4 * exact >= n, exact
    assert 2 * nonempty >= n, nonempty
    assert len(set(got)) >= 20, len(set(got))
    if scale not in (0.0, 1.0):
        k = np.float32(scale)
        clipped = sum(bool(np.any(x * k > 1) and np.any(x * k < -1)) for x in xs)
        print(f"clipped on both sides {clipped}")
        assert 4 * clipped >= 3 * n, clipped
    if scale == 0.0:
        nb = xs[0].size // bs
        both = 0
        for x in xs:
            mx = np.abs(x[:nb * bs].reshape(nb, bs)).max(axis=1).astype(np.float64)
            inv = 1 / mx[mx > 0]
            both += bool(np.any(inv > gen.MAX_SCALE) and np.any(inv < gen.MAX_SCALE))
        silent = sum(bool(np.any(np.abs(x[:nb * bs].reshape(nb, bs)).max(axis=1) == 0)) for x in xs)
        print(f"cap binds and not {both}, with a silent block {silent}")
        assert 4 * both >= n, both
        assert silent >= 1, "no stream holds an all-zero block (1 / 0, then the cap)"


def test_streams_differ():
    sr, pitch = gen.MANY_GEOMETRY[0]
    xs = gen.streams(sr, pitch, gen.MANY_STREAMS, gen.SEED)
    assert len({x.tobytes() for x in xs}) == len(xs)
    assert len(gen.TEXTS) >= 8 and len(set(gen.texts(len(xs)))) >= 8
    amp = np.array([np.abs(x).max() for x in xs])
    assert amp.min() < 0.5 and amp.max() > 1.2


# -- value regimes -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plain():
    sr, pitch = gen.REGIME_GEOMETRY
    return gen.streams(sr, pitch, gen.REGIME_STREAMS, gen.REGIME_SEED)


def regime_runs(plain, name):
    """(input, oracle magnitudes, raw) for every stream the regime is applied to, at scale 0 and scale 1."""
    sr, pitch = gen.REGIME_GEOMETRY
    bank = gen.regime_bank(name)
    for s in range(gen.REGIME_STREAMS):
        if s in gen.REGIME_ON:
            assert not np.array_equal(bank[s], plain[s], equal_nan=True)
        else:
            assert bank[s] is plain[s]
    for s in gen.REGIME_ON:
        for scale in (0.0, 1.0):
            mags, raw, _, _ = run_oracle(sr, pitch, bank[s], scale)
            yield s, scale, bank[s], mags, raw


def test_regime_subnormal(plain):
    for s, scale, x, mags, raw in regime_runs(plain, "subnormal"):
        nz = x[x != 0]
        assert np.mean(np.abs(nz) < gen.TINY) >= 1 / 3, (s, scale)
        assert nz.size * 3 >= np.count_nonzero(plain[s]), "most samples were rounded to zero"
        assert not np.any(np.isnan(mags)), (s, scale)
        assert np.mean((mags != 0) & (mags < 2.0 ** -100)) >= 1 / 3, (s, scale)


def goertzel(x, bs, coeff):
    """Goertzel.Magnitude (dsp/dsp.go:98-106) of every whole block of x, before the normalisation: the oracle returns
    magnitude / limit only, and the limit follows the magnitude (the quotient stays below 7 whatever the level), so how
    large the magnitudes themselves are is recomputed here - float64, one rounding per operation, as the oracle does."""
    nb = x.size // bs
    blocks = x[:nb * bs].reshape(nb, bs).astype(np.float64)
    q1, q2 = np.zeros(nb), np.zeros(nb)
    for i in range(bs):
        q0 = coeff * q1 - q2 + blocks[:, i]
        q2, q1 = q1, q0
    return np.sqrt((q1 * q1) + (q2 * q2) - q1 * q2 * coeff)


def normalized(mag, low):
    """NormalizedMagnitude (dsp/dsp.go:111-123) over the blocks' magnitudes."""
    out, limit = np.empty_like(mag), 0.0
    for b, m in enumerate(mag):
        if m > low:
            limit = limit + ((m - limit) / 6)
        if limit < low:
            limit = low
        out[b] = m / limit
    return out


def test_goertzel_restated(plain):
    """goertzel() above is the oracle's magnitude: normalised as the oracle normalises, it gives the oracle's bits."""
    sr, pitch = gen.REGIME_GEOMETRY
    ref = orc.AudioDemodulator(pitch, sr)
    for x in (plain[0], gen.regime(plain[2], "p127")):
        mags = run_oracle(sr, pitch, x, 1.0)[0]
        with np.errstate(all="ignore"):
            mine = normalized(goertzel(x, ref.blocksize, ref.coeff), ref.blocksize / 2)
        assert mine.tobytes() == mags.tobytes()


def test_regime_p100_and_p127(plain):
    sr, pitch = gen.REGIME_GEOMETRY
    ref = orc.AudioDemodulator(pitch, sr)
    for name in ("p100", "p127"):
        for s, scale, x, mags, raw in regime_runs(plain, name):
            assert np.all(np.isfinite(x)), f"{name} stream {s}: the multiplication overflowed"
            assert not np.any(np.isnan(mags)) and np.all(np.isfinite(mags)), (name, s, scale)
            assert np.any(raw) and not np.all(raw), (name, s, scale)
            if scale == 1.0:
                big = goertzel(x, ref.blocksize, ref.coeff)
                assert np.all(np.isfinite(big)), (name, s)
                assert np.count_nonzero(big > 2.0 ** (100 if name == "p127" else 73)) > 100, (name, s)
                if name == "p127":
                    assert big.max() > 1e39, "no magnitude beyond float32's range"


def test_regime_nonfinite(plain):
    for s, scale, x, mags, raw in regime_runs(plain, "nonfinite"):
        at = sorted(gen.NONFINITE_BLOCKS.values())
        assert np.array_equal(np.flatnonzero(~np.isfinite(mags)), at), (s, scale, np.flatnonzero(~np.isfinite(mags)))
        assert np.all(np.isnan(mags[at])) and not np.any(raw[at]), (s, scale)
        assert at[-1] + 100 < mags.size and np.any(mags[at[-1] + 1:] != 0), (s, scale)
        if scale == 0.0:  # (at scale 1 a stream below amplitude 0.75 never reaches the magnitude threshold)
            assert np.any(raw[at[-1] + 1:]), "nothing is keyed after the last planted block"


def test_regime_negzero(plain):
    for s, scale, x, mags, raw in regime_runs(plain, "negzero"):
        b, bs = gen.NEGZERO_BLOCK, gen.blocksize(*gen.REGIME_GEOMETRY)
        assert np.all(np.signbit(x[b * bs:(b + 1) * bs])) and not np.any(x[b * bs:(b + 1) * bs])
        assert mags[b] == 0 and not np.signbit(mags[b]), (s, scale, mags[b])
        assert mags[b - 1] != 0 or mags[b + 1] != 0 or np.any(mags != 0)


# -- ragged writes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs,max_blocks,n", [(39, 1024, 39 * 2482 + 17), (207, 1024, 207 * 2600), (288, 64, 288 * 300 + 1), (39, 1024, 39 * 700)])
def test_cuts(bs, max_blocks, n):
    c = gen.cuts(n, bs, max_blocks, 3)
    assert c[0] == 0 and c[-1] == n and all(a <= b for a, b in zip(c[:-1], c[1:]))
    done = gen.completed(c, bs)
    assert max(done) <= max_blocks
    lengths = [b - a for a, b in zip(c[:-1], c[1:])]
    assert 0 in lengths, "no empty write"
    assert any(0 < ln < bs and d == 0 for ln, d in zip(lengths, done)), "no write shorter than a block that completes none"
    assert any(b % bs == 0 and b > a for a, b in zip(c[:-1], c[1:])), "no write ends on a block boundary"
    if n >= (max_blocks + max_blocks // 4 + 1) * bs:
        assert max_blocks in done, "no write completes exactly max_blocks blocks"
    assert any(a % bs for a in c[1:-1]), "no write begins with samples pending"
    assert c == gen.cuts(n, bs, max_blocks, 3) and c != gen.cuts(n, bs, max_blocks, 4)


# -- text delivery ------------------------------------------------------------------------------------------------------
def test_delivery_stream_runes():
    x, bs = gen.delivery_stream(gen.DELIVERY_BLOCKS_LONG)
    assert bs == 39
    text = gen.delivery_oracle(x)
    assert len(text) > gen.TEXT_CAP and set(text) == {"§"}, (len(text), sorted(set(text)))
    short = gen.delivery_oracle(x[:gen.DELIVERY_BLOCKS_SHORT * bs])
    assert len(short) == 1875 and text.startswith(short)
    assert len(short.encode()) == 2 * len(short)
