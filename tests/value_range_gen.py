"""Streams whose psd words sit anywhere in the float32 range: the generator of tests/test_value_range_host.py (which checks,
on the oracle's own numbers, that every regime is what its name says) and tests/test_value_range_gpu.py (which runs them
through the bank).  Pure numpy and the oracle; a plain helper module, not a test file.

A regime is defined by where the ORACLE's psd lands, not by a constant: the unscaled stream's psd is sampled (mean of the
noise words `m`, strongest word `c`) and the power of two 2^k that the samples are multiplied by is chosen so that m * 4^k
(or c * 4^k) lies where the regime says.  A noise word is exponentially distributed about its mean, so the share of words
that round to zero (below 2^-150) or overflow (from 2^128 on) follows from the mean alone:

  low          m -> [2^-139, 2^-137): nearly every word subnormal (a word in 4000 rounds to 0), everything alive
  floor        m -> [2^-148, 2^-146): words are small multiples of 2^-149, 6 - 22 % of them zero; means non-zero
  zero_edge    the first k below floor's at which a window's mean rounds to exactly 0 in a sampled frame
  high         c -> (2^125.5, 2^127.5]: everything finite, the carriers just under overflow
  carrier_inf  m -> [2^112, 2^114): the carriers (2^19 above) are +Inf, the largest noise word stays below 2^120
  noise_inf    m -> [2^126, 2^128): 2 - 37 % of the noise words +Inf
  all_inf      m -> [2^129, 2^131): 61 - 88 % of the words +Inf, every window holds one
  breathing    the exponent changes with every frame: a triangle of 100 frames between m -> [2^-120, 2^-118) (no word of these
               streams rounds to zero there) and high's k, so that one cumulation sums dB values 670 dB apart

The carriers' amplitude is 0.04 * sqrt(512 / N): the ratio c / m is then 2^19.2 at every block size, a regime looks the
same at every N, and floor's carriers (below 2^-126.8) are subnormal like everything else in it.  The multiplication by
2^k is exact (no sample of these streams is below 2^-40, so none becomes subnormal), and the float64 FFT neither
overflows nor underflows: only the float32 rounding of the psd changes."""
import functools
import math
from typing import NamedTuple

import numpy as np

from oracle import oracle as orc
from sdrainer_amd import synth

REGIMES = ("low", "floor", "zero_edge", "high", "carrier_inf", "noise_inf", "all_inf", "breathing")
RATES = {n: 48_000 * n // 512 for n in (512, 8192, 16384, 32768, 65536)}  # a frame is 10.7 ms and a dit 6 frames at every N: 230 frames hold text
TONES = {512: 3, 8192: 8, 16384: 8, 32768: 8, 65536: 8}  # (N = 512: three, as where the regimes were first measured)
TEXT = "se5 de ei5sh ei5sh e"  # keyed down two thirds of the time: a +Inf carrier leaves its noise window free in most frames
BREATH_PERIOD = 100  # frames: the cumulation's length, so that every cumulation holds a whole walk up and down
# the walk is lowest at frames 45, 145 ...: FindPeaks compares a cumulation (frames 0 - 99) with the rolling noise floor of its
# last 60 frames (40 - 99), and about frame 70, halfway up, those 60 frames have the mean of all 100 - the carriers are
# then the peaks.  Lowest at frame 0 the threshold lies 45 dB above every bin (no peak), lowest at 60 below (one peak, 0 - N-1)
BREATH_LOWEST = 45
SAMPLED = 13  # psd statistics come from frames 0, 13, 26 ...


TINY = np.float32(2.0 ** -126)  # the smallest normal float32


def subnormal(x):
    return (x > 0) & (x < TINY)


def amplitude(n):
    return 0.04 * math.sqrt(512.0 / n)


@functools.lru_cache(maxsize=3)
def base(n, frames, seed):
    """The unscaled stream (float32 [frames, 2N], read-only) and its carriers' bins."""
    iq, bins, _ = synth.make_band(frames, RATES[n], n, TONES[n], seed=seed, amplitude=amplitude(n), text=TEXT)
    iq.setflags(write=False)
    return iq, [int(b) for b in bins]


def noise_mask(n, bins):
    """True at every bin that is no carrier and no neighbour of one."""
    mask = np.ones(n, bool)
    for b in bins:
        mask[max(0, b - 1):b + 2] = False
    return mask


def sampled_psd(iq, n):
    """The oracle's psd rows of frames 0, 13, 26 ... as float64 [rows, N] (of the UNSCALED stream: nothing rounds away)."""
    return np.stack([orc.iq_to_spectrum_and_psd(iq[f])[1] for f in range(0, iq.shape[0], SAMPLED)]).astype(np.float64)


def _k_for(value, lo):
    """The k that puts value * 4^k into [2^lo, 2^(lo + 2))."""
    return math.ceil((lo - math.log2(value)) / 2)


def _k_high(c):
    return math.floor((127.5 - math.log2(c)) / 2)


def _k_zero_edge(iq, n, edge, k_floor):
    """The first k below floor's at which a sampled frame has min_mean == 0 and non-zero words."""
    for k in range(k_floor - 1, k_floor - 8, -1):
        for f in range(0, iq.shape[0], SAMPLED):
            _, psd = orc.iq_to_spectrum_and_psd(scale(iq[f], k))
            if np.any(psd) and orc.find_noise_floor(psd, edge)[0] == 0:
                return k
    raise AssertionError("no exponent gives a window mean of exactly zero beside non-zero words")


def scale(x, k):
    """x * 2^k in float32, k an int or one int per frame (|k| may exceed float32's exponent range: in two steps)."""
    k = np.asarray(k, np.int64)
    h = k // 2
    a = np.ldexp(np.float32(1), h).astype(np.float32)
    b = np.ldexp(np.float32(1), k - h).astype(np.float32)
    if k.ndim:
        a, b = a[:, None], b[:, None]
    return ((x * a).astype(np.float32) * b).astype(np.float32)


def exponents(regime, n, frames, seed, iq=None, bins=None, edge=None):
    """The regime's k for the stream (n, frames, seed), or for the given unscaled frames (a windowed stream): an int, or
    for breathing an int64 per frame."""
    if iq is None:
        iq, bins = base(n, frames, seed)
    edge = synth.default_edge_width(n) if edge is None else edge
    psd = sampled_psd(iq, n)
    m = float(psd[:, noise_mask(n, bins)].mean())
    c = max(float(psd.max()), (amplitude(n) * n) ** 2 * 1.01)
    if regime == "low":
        return _k_for(m, -139)
    if regime == "floor":
        return _k_for(m, -148)
    if regime == "zero_edge":
        return _k_zero_edge(iq, n, edge, _k_for(m, -148))
    if regime == "high":
        return _k_high(c)
    if regime == "carrier_inf":
        return _k_for(m, 112)
    if regime == "noise_inf":
        return _k_for(m, 126)
    if regime == "all_inf":
        return _k_for(m, 129)
    assert regime == "breathing", regime
    lo, hi = _k_for(m, -120), _k_high(c)
    phase = (np.arange(frames) - BREATH_LOWEST) % BREATH_PERIOD
    tri = np.minimum(phase, BREATH_PERIOD - phase) / (BREATH_PERIOD // 2)  # 0 ... 1 ... 0
    return lo + np.rint((hi - lo) * tri).astype(np.int64)


def band(regime, n, frames, seed):
    """One band as parity_case.Case(bands=...) takes it: (float32 [frames, 2N], None, the carriers' bins)."""
    iq, bins = base(n, frames, seed)
    return scale(iq, exponents(regime, n, frames, seed)), None, bins


def listeners(n, bins):
    """The carriers, both neighbours of each, bins 0 and N - 1, and a noise bin."""
    out = list(bins)
    for b in bins:
        out += [b - 1, b + 1]
    noise = (bins[0] + bins[1]) // 2
    assert all(0 < b < n - 1 for b in out) and noise_mask(n, bins)[noise] and noise_mask(n, bins)[0] and noise_mask(n, bins)[n - 1]
    return out + [0, n - 1, noise]


class Spec(NamedTuple):
    """One GPU case: `kernel` names the FFT kernel the geometry picks (the id only), `batches` the frames per batch
    (a batch of 1, batches below 100 frames, one across a cumulation boundary), `env` the switches the bank is created
    under."""
    kernel: str
    regime: str
    n: int
    n_bands: int
    path: str
    batches: tuple
    env: tuple = ()

    @property
    def id(self):
        return f"{self.kernel}-{self.regime}"

    @property
    def frames(self):
        return sum(self.batches)

    def seed(self, b=0):
        return 9000 + self.n // 64 + 17 * b

    def bands(self):
        return [band(self.regime, self.n, self.frames, self.seed(b)) for b in range(self.n_bands)]


# what the batch plan (csrc/host/batch_plan.h) must choose for the cases of a kernel id: k_fft_r32 and its wide tap in the
# launch of 1030 frames only, the two-phase FFT above N = 16384, the one-pass noise scan up to 16384 and the chains above
PLAN = {"psd9": dict(r32=0, two_phase=0, noise_scan=1), "psd13": dict(r32=0, two_phase=0, noise_scan=1),
        "psd14": dict(r32=0, two_phase=0, noise_scan=1), "r32": dict(r32=1, wide_tap=1, two_phase=0, noise_scan=1),
        "2p32768": dict(r32=0, two_phase=1, noise_scan=0), "2p65536": dict(r32=0, two_phase=1, noise_scan=0)}

SHORT = (1, 60, 120, 49)  # 230 frames
R32 = (1, 40, 1030, 129)  # 1200 frames: one launch of 1030, k_fft_psd<14> around it
GROUPS = (("SDR_FFT2P_GROUP_MB", "32"),)  # 64 (N = 32768) and 32 (N = 65536) frames per group: the batch of 120 spans several

MATRIX = (
    [Spec("psd9", r, 512, 2, "device", (1, 70, 130, 59)) for r in REGIMES]
    + [Spec("psd13", r, 8192, 1, "staged", SHORT) for r in ("low", "floor", "carrier_inf", "breathing")]
    + [Spec("psd14", r, 16384, 1, "device", SHORT) for r in ("floor", "carrier_inf", "breathing")]
    + [Spec("r32", r, 16384, 1, "device", R32) for r in ("low", "floor", "carrier_inf", "noise_inf", "breathing")]
    + [Spec("2p32768", r, 32768, 1, "device", SHORT, GROUPS) for r in ("floor", "carrier_inf", "breathing", "all_inf")]
    + [Spec("2p65536", r, 65536, 1, "device", SHORT, GROUPS) for r in ("floor", "carrier_inf", "breathing")]
)
# the cases tests/test_forced_paths.py runs under the other implementations of the noise floor and the cumulation
FORCED = [s.id for s in MATRIX if s.kernel == "psd9" or (s.kernel == "r32" and s.regime in ("floor", "carrier_inf"))]

NAN_OK = ("zero_edge", "carrier_inf", "noise_inf", "all_inf")
ACTIVE = ("low", "breathing")


# -- windowed input -----------------------------------------------------------------------------------------------------
class WSpec(NamedTuple):
    """One windowed case (dense frames, hop = 0): the oracle is fed float32(x[i] * w[i]).  float32 input: samples and
    table each carry half of the exponent; sc16: the table carries all of it."""
    kernel: str
    regime: str
    n: int
    sc16: bool
    batches: tuple = SHORT

    @property
    def id(self):
        return f"{self.kernel}-{self.regime}"


WINDOWED = (
    [WSpec("psd_win9", r, 512, False) for r in ("low", "floor")]
    + [WSpec("psd_sc16_win9", r, 512, True) for r in ("low", "floor")]
    + [WSpec("fft2p_win_a", r, 32768, False) for r in ("low", "floor")]
)


def windowed_input(spec):
    """(float32 stream [samples, 2], int16 stream or None, float32 window [N], the carriers' bins): the window is one period
    of a sine about 0.6 with a phase of 1 rad (0.25 - 0.95, not symmetric: a reversed or shifted index changes every
    product; its leakage stays in the carriers' neighbours, so the noise bins keep their level - a random table spreads a
    keyed carrier over every bin, and the floor then jumps by 2^7 with the keying) times a power of two, and the regime is
    placed on the psd of the WINDOWED frames."""
    n, frames = spec.n, sum(spec.batches)
    iq, bins = base(n, frames, 9500 + n // 64)
    s, q = iq.reshape(-1, 2), None
    if spec.sc16:
        q = np.rint(s.astype(np.float64) * (30000.0 / float(np.abs(s).max()))).astype(np.int16)
        s = q.astype(np.float32) / np.float32(32767.0)
    w = (0.6 + 0.35 * np.sin(2.0 * np.pi * np.arange(n) / n + 1.0)).astype(np.float32)
    plain = (s.reshape(-1, n, 2) * w[None, :, None]).astype(np.float32).reshape(-1, 2 * n)
    k = exponents(spec.regime, n, frames, 0, iq=plain, bins=bins)
    ks = 0 if spec.sc16 else k // 2
    s = s if spec.sc16 else scale(s, ks)
    return s, q, scale(w, k - ks), bins
