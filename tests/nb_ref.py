"""The impulse noise blanker's arithmetic restated in NumPy and Python integers, written from the text of
include/sdrainer_hip.h "impulse noise blanker": the oracle of tests/test_nb_ref.py, test_nb_gpu.py and test_nb_c.py.  Every
quantity is an exact integer (block powers in uint64, the two sides of the inequality in Python integers, which cannot
wrap).  A plain helper module, not a test file."""
import numpy as np

SC16, CS8, CU8 = 1, 2, 3
REAL = 16
RS16, RS8, RU8 = REAL | SC16, REAL | CS8, REAL | CU8
FORMATS = (SC16, CS8, CU8, RS16, RS8, RU8)
FORMAT_IDS = ("sc16", "cs8", "cu8", "rs16", "rs8", "ru8")
RAW_DTYPE = {SC16: np.int16, CS8: np.int8, CU8: np.uint8, RS16: np.int16, RS8: np.int8, RU8: np.uint8}


def is_real(fmt):
    return bool(fmt & REAL)


def units(raw, fmt):
    """int64 units u of raw values: x for int8 and int16, 2 x - 255 for uint8."""
    x = np.asarray(raw, RAW_DTYPE[fmt]).astype(np.int64)
    return 2 * x - 255 if (fmt & ~REAL) == CU8 else x


def mags(raw, fmt):
    """m[k], int64 [n]: uI^2 + uQ^2 of a complex sample [n, 2], u^2 of a real one [n]."""
    u = units(raw, fmt)
    if is_real(fmt):
        assert u.ndim == 1
        return u * u
    assert u.ndim == 2 and u.shape[1] == 2
    return u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]


def blank_words(k, fmt):
    """The blank words of the samples with absolute indices k (int64 [n]), in the format's raw dtype."""
    par = (np.asarray(k, np.int64) & 1).astype(np.int64)
    if (fmt & ~REAL) != CU8:
        shape = (len(par),) if is_real(fmt) else (len(par), 2)
        return np.zeros(shape, RAW_DTYPE[fmt])
    if is_real(fmt):
        return (127 + par).astype(np.uint8)
    return np.stack([127 + par, 128 - par], axis=1).astype(np.uint8)


def random_raw(n, fmt, seed, spread=None):
    """n raw samples over the format's whole range ([n, 2] complex, [n] real); spread: a smaller range around the centre."""
    rng = np.random.default_rng(seed)
    info = np.iinfo(RAW_DTYPE[fmt])
    lo, hi = (info.min, info.max + 1) if spread is None else ((info.min + info.max + 1) // 2 - spread, (info.min + info.max + 1) // 2 + spread + 1)
    shape = (n,) if is_real(fmt) else (n, 2)
    return rng.integers(lo, hi, shape).astype(RAW_DTYPE[fmt])


def full_scale(fmt):
    """The raw word of the largest m."""
    info = np.iinfo(RAW_DTYPE[fmt])
    v = info.min if info.min < 0 else info.max
    return v if is_real(fmt) else (v, v)


class NbRef:
    """One blanker: process(raw) takes the next len(raw) (a multiple of B) raw samples and returns the blanked ones.  It
    keeps the last W block powers, the number of blocks seen and the last impulse's gate; `stats` are the totals since
    the last read_stats()."""

    def __init__(self, fmt, block, window, ratio_q4, hold, first_sample=0):
        assert first_sample % block == 0 and 0 <= hold <= block
        self.fmt, self.B, self.W = fmt, int(block), int(window)
        self.ratio_q4, self.hold = int(ratio_q4), int(hold)
        self.k = int(first_sample)   # absolute index of the next sample
        self.blocks = 0              # blocks seen since the start
        self.powers = []             # the last W block powers, Python integers
        self.gate_end = -1           # absolute index of the last sample of the open gate (below self.k: closed)
        self.stats = dict(samples=0, impulses=0, blanked=0, reserved=0)

    def set_threshold(self, ratio_q4, hold):
        assert 0 <= hold <= self.B
        self.ratio_q4, self.hold = int(ratio_q4), int(hold)

    def read_stats(self):
        s, self.stats = self.stats, dict(samples=0, impulses=0, blanked=0, reserved=0)
        return s

    def process(self, raw):
        raw = np.asarray(raw, RAW_DTYPE[self.fmt])
        n, B, W = len(raw), self.B, self.W
        assert n > 0 and n % B == 0
        m = mags(raw, self.fmt)
        span = B * W
        impulse = np.zeros(n, bool)
        for j in range(n // B):
            mj = m[j * B:(j + 1) * B]
            if self.blocks >= W and self.ratio_q4 != 0:
                R = sum(self.powers)
                # m * (B W) * 16 > ratio_q4 * R, both sides exact: the largest left side is below 2^52
                rhs = self.ratio_q4 * R
                impulse[j * B:(j + 1) * B] = np.array([int(v) * span * 16 > rhs for v in mj]) if rhs >= 2 ** 62 else \
                    mj.astype(np.uint64) * np.uint64(span * 16) > np.uint64(rhs)
            self.powers = (self.powers + [int(mj.sum())])[-W:]
            self.blocks += 1
        # the gate: sample k is blanked iff an impulse i has i <= k <= i + hold (this call's hold), or the gate left open
        # by an earlier call still covers it
        idx = np.arange(n, dtype=np.int64)
        last = np.maximum.accumulate(np.where(impulse, idx, np.int64(-1) << 40))
        blanked = (idx - last <= self.hold) | (idx + self.k <= self.gate_end)
        out = raw.copy()
        out[blanked] = blank_words(idx[blanked] + self.k, self.fmt)
        if impulse.any():
            self.gate_end = max(self.gate_end, self.k + int(idx[impulse][-1]) + self.hold)
        self.k += n
        self.stats["samples"] += n
        self.stats["impulses"] += int(impulse.sum())
        self.stats["blanked"] += int(blanked.sum())
        return out


def nb_ref(raw, fmt, block, window, ratio_q4, hold):
    """The whole stream in one call from k = 0: (blanked samples, stats)."""
    ref = NbRef(fmt, block, window, ratio_q4, hold)
    return ref.process(raw), ref.read_stats()


def add_stats(a, b):
    return {f: a[f] + b[f] for f in a}
