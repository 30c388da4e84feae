"""Input of the Goertzel audio path's tests: the generator of tests/test_audio_host.py (which checks, on the oracle's own
numbers, that every case is what its name says) and tests/test_audio_gpu.py (which runs the cases through sdr_audio_*).
Pure numpy and the oracle; a plain helper module, not a test file.

A bank's streams differ in everything a lane of k_audio_decode can differ in: text, speed, amplitude (0.2 - 1.5: above 1 a
scale of 1 leaves samples beyond +-1 unclipped, a scale of 2.5 or -3 clips nearly every stream on both sides), phase, where
in a block the keying starts, and noise (none, so that key-up blocks are exactly 0 and autoscale meets 1 / 0; 0.01 and
0.05, so that key-up blocks reach the maxScale cap at max > 0; 0.2, so that the decoder sees keying it cannot name)."""
import functools

import numpy as np

from oracle import oracle as orc

TEXTS = ("cq de dl1abc", "5nn tu", "test w1aw", "cq cq dx", "r 599 k", "de ei5sh k", "qrz? ly2px", "73 es gl", "ii3wwa tu 5nn",
         "gb4wwa test", "sos sos", "vvv de oh2b", "qth paris", "ur rst 579", "pse k", "cq test n0ax")
NOISE = (0.0, 0.01, 0.05, 0.2)
SCALES = (0.0, 1.0, 2.5, -3.0)
MAX_SCALE = 12.0  # cw/audio.go defaultMaxScale
TINY = np.float32(2.0 ** -126)  # the smallest normal float32

# sample rate, pitch, the oracle's blocksize (literal: tests/test_audio_host.py holds the oracle to them)
GEOMETRY = (
    (48000, 700.0, 207),
    (8000, 600.0, 39),
    (12000, 800.0, 60),
    (44100, 443.0, 200),
    (11025, 700.0, 48),
    (48000, 500.0, 288),  # 240 / 96 = 2.5 rounds away from zero, to 3
    (8000, 640.0, 39),    # 8000 / 640 = 12.5 rounds to 13
    (16000, 1000.0, 80),
    (8000, 30.0, 0),      # round(40 / 267) = 0: no block, sdr_audio_create refuses it
)
MANY_GEOMETRY = ((8000, 600.0), (11025, 700.0), (12000, 800.0))
MANY_STREAMS = 130  # 64 + 64 + 2: two whole workgroups of k_audio_decode and a wave with two lanes
# (sample rate, pitch, streams, scale) of every case the GPU test runs with many streams
MANY = tuple((sr, p, MANY_STREAMS, sc) for sr, p in MANY_GEOMETRY for sc in SCALES) + ((8000, 600.0, 65, 0.0), (11025, 700.0, 1, 2.5))
SMALL_GEOMETRY = tuple(g for g in GEOMETRY if g[2] and g[:2] not in MANY_GEOMETRY)
SEED = 77

REGIMES = ("subnormal", "p100", "p127", "nonfinite", "negzero")
NONFINITE_BLOCKS = {"+inf": 310, "-inf": 700, "nan": 1100}  # far enough apart for the decoder to settle between them
NEGZERO_BLOCK = 777
REGIME_GEOMETRY = (8000, 600.0)
REGIME_STREAMS = 5  # the regime on streams 0, 2, 3; streams 1 and 4 stay as they are
REGIME_ON = (0, 2, 3)
REGIME_SEED = 25

# text delivery: debounce 1 and 2 blocks on, 2 blocks off is keying the decoder has no name for - one U+00A7 per 32 blocks
DELIVERY_GEOMETRY = (8000, 600.0)
DELIVERY_BLOCKS_SHORT = 60000  # 1875 runes
DELIVERY_BLOCKS_LONG = 140000  # more than the 4096 a stream stores
TEXT_CAP = 4096


def blocksize(sample_rate, pitch):
    return orc.AudioDemodulator(pitch, sample_rate).blocksize


@functools.lru_cache(maxsize=4)
def streams(sample_rate, pitch, n_streams, seed):
    """n_streams float32 arrays (read-only) of equal length: keyed tones at `pitch`, each with its own text, speed, amplitude,
    phase, start offset within a block and noise; the shorter ones padded with zeros."""
    bs = blocksize(sample_rate, pitch)
    rng = np.random.default_rng([seed, sample_rate, n_streams])
    made = []
    for s in range(n_streams):
        text = TEXTS[(s + 5 * (s // len(TEXTS))) % len(TEXTS)]
        wpm = int(rng.integers(14, 36))
        amplitude = float(rng.uniform(0.2, 1.5))
        phase = float(rng.uniform(0, 2 * np.pi))
        offset = int(rng.integers(0, bs))
        sigma = NOISE[int(rng.integers(0, len(NOISE)))]
        key = np.repeat(orc.generate_stream(sample_rate, bs, wpm, text), bs).astype(np.float64)
        env = np.concatenate([np.zeros(offset), key])
        t = np.arange(env.size) / sample_rate
        x = amplitude * np.cos(2 * np.pi * pitch * t + phase) * env
        noise = rng.standard_normal(env.size)  # drawn for every stream, so that a stream does not depend on its neighbours' noise
        made.append((text, wpm, (x + sigma * noise).astype(np.float32)))
    n = max(x.size for _, _, x in made)
    out = []
    for _, _, x in made:
        y = np.zeros(n, np.float32)
        y[:x.size] = x
        y.setflags(write=False)
        out.append(y)
    return tuple(out)


def texts(n_streams):
    """The text keyed into each stream of streams(..., n_streams, ...)."""
    return [TEXTS[(s + 5 * (s // len(TEXTS))) % len(TEXTS)] for s in range(n_streams)]


def regime(x, name, blocksize=None):
    """The stream changed as the regime says (a copy).  The multiplications are by powers of two, in float32: 2^-130 leaves
    every sample below the smallest normal (those below 2^-20 become 0), 2^100 and 2^127 are exact."""
    x = np.array(x, np.float32)
    if name == "subnormal":
        return (x * np.float32(2.0 ** -65)).astype(np.float32) * np.float32(2.0 ** -65)
    if name == "p100":
        return x * np.float32(2.0 ** 100)
    if name == "p127":
        return x * np.float32(2.0 ** 127)
    mid = blocksize // 2  # mid-block: a non-finite sample in the last place of a block can leave q1 * q1 = +Inf, not NaN
    if name == "nonfinite":
        for kind, b in NONFINITE_BLOCKS.items():
            x[b * blocksize + mid] = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan}[kind]
        return x
    assert name == "negzero", name
    x[NEGZERO_BLOCK * blocksize:(NEGZERO_BLOCK + 1) * blocksize] = np.float32(-0.0)
    return x


def regime_bank(name):
    """The five streams of a regime's bank."""
    sr, pitch = REGIME_GEOMETRY
    bs = blocksize(sr, pitch)
    return [regime(x, name, bs) if s in REGIME_ON else x for s, x in enumerate(streams(sr, pitch, REGIME_STREAMS, REGIME_SEED))]


def cuts(n_samples, blocksize, max_blocks, seed):
    """Ragged write boundaries 0 = c[0] <= c[1] ... <= c[-1] = n_samples; no write completes more than max_blocks blocks.
    As far as n_samples reaches they begin with a write shorter than a block, an empty one, one that ends exactly on a
    block boundary and one that completes exactly max_blocks blocks (and leaves a remainder); random lengths follow."""
    rng = np.random.default_rng([seed, n_samples, blocksize, max_blocks])
    c = [0]

    def add(to):
        if c[-1] <= to <= n_samples:
            c.append(int(to))

    add(max(1, blocksize // 2) if blocksize > 1 else 0)
    add(c[-1])
    add(blocksize * int(rng.integers(2, max(3, max_blocks // 4))))
    if c[-1] % blocksize == 0:
        add(c[-1] + max_blocks * blocksize + int(rng.integers(1, max(2, blocksize))) % blocksize)
    while c[-1] < n_samples:
        pending = c[-1] % blocksize
        room = max_blocks * blocksize + (blocksize - 1) - pending  # the longest write that completes max_blocks blocks
        c.append(min(n_samples, c[-1] + int(rng.integers(0, room + 1))))
    return c


def completed(c, blocksize):
    """Blocks completed by each write of cuts c."""
    return [b // blocksize - a // blocksize for a, b in zip(c[:-1], c[1:])]


def delivery_stream(n_blocks):
    """One stream of n_blocks blocks, 2 blocks of tone and 2 of silence in turn, and its blocksize."""
    sr, pitch = DELIVERY_GEOMETRY
    bs = blocksize(sr, pitch)
    env = np.repeat((np.arange(n_blocks) % 4 < 2).astype(np.float32), bs)
    t = np.arange(env.size) / sr
    return (0.8 * np.cos(2 * np.pi * pitch * t) * env).astype(np.float32), bs


def delivery_oracle(x):
    sr, pitch = DELIVERY_GEOMETRY
    ref = orc.AudioDemodulator(pitch, sr)
    ref.set_debounce(1)
    ref.write(x)
    ref.close()
    return ref.text()
