"""The down-converter's arithmetic restated in NumPy (include/sdrainer_hip.h "down-converter"): the
oracle of tests/test_ddc_ref.py, test_ddc_gpu.py and test_ddc_c.py.  Every array operation below is one float32 operation
per element, rounded once, which is the contract; the NCO table is an argument (capi.ddc_nco_table(): libm and NumPy may
differ in the last place, so the tests never recompute it).  A plain helper module, not a test file."""
import numpy as np

from sdrainer_amd import synth

L = 65536
F32, SC16, CS8, CU8 = range(4)
FORMATS = (F32, SC16, CS8, CU8)
FORMAT_IDS = ("f32", "sc16", "cs8", "cu8")
RAW_DTYPE = {F32: np.float32, SC16: np.int16, CS8: np.int8, CU8: np.uint8}


def to_f32(raw, fmt):
    """The float32 values of raw samples [n, 2]: exact for the 8-bit formats, float32(x) / 32767 rounded once for sc16."""
    raw = np.asarray(raw, RAW_DTYPE[fmt])
    if fmt == F32:
        return raw
    if fmt == SC16:
        return raw.astype(np.float32) / np.float32(32767.0)
    if fmt == CS8:
        return raw.astype(np.float32) / np.float32(128.0)
    return (raw.astype(np.float32) * np.float32(2.0) - np.float32(255.0)) / np.float32(256.0)


def random_raw(n, fmt, seed):
    """n raw samples [n, 2] over the format's whole range (float32: uniform in [-1, 1))."""
    rng = np.random.default_rng(seed)
    if fmt == F32:
        return (rng.random((n, 2), dtype=np.float32) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    info = np.iinfo(RAW_DTYPE[fmt])
    return rng.integers(info.min, info.max + 1, (n, 2)).astype(RAW_DTYPE[fmt])


def mix(x, k, step, cos, sin):
    """y [n, 2] float32 of samples x [n, 2] float32 at stream indices k (int64) for one band's step."""
    p = (k * np.int64(step)) & np.int64(L - 1)  # two's complement: the mathematical (k * step) mod L for either sign
    c, s = cos[p], sin[p]
    re, im = x[:, 0], x[:, 1]
    return np.stack([(re * c) + (im * s), (im * c) - (re * s)], axis=1)


class DdcRef:
    """One DDC: process(x) takes the next len(x) (a multiple of D) float32 samples [n, 2] and returns float32
    [bands, n / D, 2].  It keeps the last T - 1 RAW samples and mixes them again from their absolute index with the steps
    current in the call; samples below the first sample are zero."""

    def __init__(self, decimation, taps, steps, cos, sin, first_sample=0):
        self.d, self.taps, self.steps = int(decimation), np.asarray(taps, np.float32), [int(s) for s in steps]
        self.cos, self.sin = np.asarray(cos, np.float32), np.asarray(sin, np.float32)
        self.total = int(first_sample)
        self.hist = np.zeros((len(self.taps) - 1, 2), np.float32)

    def process(self, x):
        x = np.asarray(x, np.float32).reshape(-1, 2)
        d, t = self.d, len(self.taps)
        assert len(x) % d == 0 and self.total % d == 0
        m = len(x) // d
        span = np.concatenate([self.hist, x])
        k = self.total - (t - 1) + np.arange(len(span), dtype=np.int64)
        at = (t - 1) + np.arange(m) * d  # span index of sample n * D of output n
        out = np.empty((len(self.steps), m, 2), np.float32)
        for b, step in enumerate(self.steps):
            y = mix(span, k, step, self.cos, self.sin)
            acc = np.zeros((m, 2), np.float32)
            for j in range(t):
                acc = acc + (self.taps[j] * y[at - j])
            out[b] = acc
        self.hist = span[len(span) - (t - 1):]
        self.total += len(x)
        return out


def ddc_ref(x, decimation, taps, steps, cos, sin, first_sample=0):
    """The whole stream in one call."""
    return DdcRef(decimation, taps, steps, cos, sin, first_sample).process(x)


def ddc_f64(x, decimation, taps, steps, cos, sin):
    """The same sums evaluated directly in float64 (the table's float32 values, no intermediate rounding), and max |y|."""
    x = np.asarray(x, np.float64).reshape(-1, 2)
    d, t = int(decimation), len(taps)
    m = len(x) // d
    span = np.concatenate([np.zeros((t - 1, 2)), x])
    k = np.arange(len(span), dtype=np.int64) - (t - 1)
    at = (t - 1) + np.arange(m) * d
    h = np.asarray(taps, np.float64)
    out = np.empty((len(steps), m, 2))
    ymax = 0.0
    for b, step in enumerate(steps):
        p = (k * np.int64(step)) & np.int64(L - 1)
        z = (span[:, 0] + 1j * span[:, 1]) * (cos[p].astype(np.float64) - 1j * sin[p].astype(np.float64))
        ymax = max(ymax, float(np.abs(z).max()))
        acc = np.zeros(m, np.complex128)
        for j in range(t):
            acc += h[j] * z[at - j]
        out[b, :, 0], out[b, :, 1] = acc.real, acc.imag
    return out, ymax


# -- the end-to-end fixture: one cu8 wide stream, two keyed call signs in two segments (test_ddc_ref.py pins its oracle half,
#    test_ddc_gpu.py runs DDC and bank) ---------------------------------------------------------------------------------------
E2E = dict(wide_rate=384_000, decimation=8, taps_per_phase=8, n=512, hop=128, rate=48_000, edge=70, steps=(9000, -20000),
           bins=(320, 224), texts=("dl1abc dl1abc", "w1aw w1aw w1aw"), calls=("dl1abc", "w1aw"), dit_ticks=(8, 10),
           amplitude=0.3, sigma=0.02, frames=1800, seed=77)


def e2e_wide():
    """(cu8 [samples, 2], narrow samples per band): the carriers sit on bins E2E["bins"] of their bands' N-point spectra."""
    e = E2E
    narrow = (e["frames"] - 1) * e["hop"] + e["n"]
    narrow += -narrow % 4
    wide = narrow * e["decimation"]
    carriers = []
    for step, bin_, text, dit in zip(e["steps"], e["bins"], e["texts"], e["dit_ticks"]):
        offset = step * e["wide_rate"] / L + (bin_ - e["n"] // 2) * e["rate"] / e["n"]
        per_tick = e["hop"] * e["decimation"]
        key = np.repeat(np.concatenate([np.zeros(40, np.uint8), synth.keying_pattern(text, dit)]), per_tick)
        carriers.append((offset, e["amplitude"], key))
    return synth.wide_stream(wide, e["wide_rate"], carriers, noise_sigma=e["sigma"], seed=e["seed"], quantise="cu8"), narrow


def e2e_taps():
    return synth.lowpass_taps(E2E["decimation"], E2E["taps_per_phase"])
