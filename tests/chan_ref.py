"""The polyphase channelizer's arithmetic restated in NumPy (include/sdrainer_hip.h "channelizer"): the
oracle of tests/test_chan_ref.py, test_chan_gpu.py and test_chan_c.py.  Every array operation below is one float32 operation
per element, rounded once, which is the contract; the table is an argument (capi.ddc_nco_table()), as in tests/ddc_ref.py,
whose formats and conversions are used as they are.  A plain helper module, not a test file."""
import numpy as np

import ddc_real as RR
import ddc_ref as R
from sdrainer_amd import synth

L = R.L
# every input format: (format, id, is real)
FORMATS = tuple(R.FORMATS) + tuple(RR.FORMATS)
FORMAT_IDS = tuple(R.FORMAT_IDS) + tuple(RR.FORMAT_IDS)


def is_real(fmt):
    return bool(fmt & RR.REAL)


def random_raw(n, fmt, seed):
    """n raw samples of the format: [n, 2] for a complex one, [n] for a real one."""
    return RR.random_raw_real(n, fmt, seed) if is_real(fmt) else R.random_raw(n, fmt, seed)


def to_f32(raw, fmt):
    """float32 [n, 2] of raw samples of either kind: a real value v is (v, +0.0)."""
    return RR.as_complex(RR.to_f32_real(raw, fmt)) if is_real(fmt) else R.to_f32(raw, fmt)


def bitrev(m):
    bits = m.bit_length() - 1
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) if bits else 0 for i in range(m)], np.int64)


def fft_plus(v, cos, sin):
    """v [m, M, 2] float32 -> the unnormalised M-point transform with kernel e^{+j 2 pi c r / M} of every row: radix 2,
    decimation in time, twiddles (cos, sin)[q L / len], every twiddle multiplied, every operation rounded on its own."""
    M = v.shape[1]
    a = v[:, bitrev(M)].copy()
    ln = 2
    while ln <= M:
        h = ln // 2
        q = np.arange(h)
        wr, wi = cos[q * (L // ln)], sin[q * (L // ln)]
        a = a.reshape(a.shape[0], M // ln, ln, 2)
        lo, hi = a[:, :, :h], a[:, :, h:]
        t = np.stack([(wr * hi[..., 0]) - (wi * hi[..., 1]), (wr * hi[..., 1]) + (wi * hi[..., 0])], -1)
        a = np.concatenate([lo + t, lo - t], 2).reshape(a.shape[0], M, 2)
        ln *= 2
    return a


class ChanRef:
    """One channelizer: process(x) takes the next len(x) (a multiple of D) float32 samples [n, 2] and returns float32
    [streams, n / D, 2], stream i being channel channels[i].  It keeps the last T - 1 RAW samples and the absolute index of
    the next sample; samples below the first sample are zero."""

    def __init__(self, n_channels, decimation, taps, cos, sin, channels=None, first_sample=0):
        self.m, self.d, self.taps = int(n_channels), int(decimation), np.asarray(taps, np.float32)
        assert len(self.taps) % self.m == 0 and first_sample % self.d == 0
        self.cos, self.sin = np.asarray(cos, np.float32), np.asarray(sin, np.float32)
        self.channels = list(range(self.m)) if channels is None else [int(c) for c in channels]
        self.total = int(first_sample)
        self.hist = np.zeros((len(self.taps) - 1, 2), np.float32)

    def process(self, x):
        x = np.asarray(x, np.float32).reshape(-1, 2)
        M, d, t = self.m, self.d, len(self.taps)
        assert len(x) % d == 0
        m = len(x) // d
        span = np.concatenate([self.hist, x])
        at = (t - 1) + np.arange(m) * d                                # span index of sample n * D of output time n
        nd = np.int64(self.total) + np.arange(m, dtype=np.int64) * d   # n * D, the full index
        r = np.arange(M)
        u = np.zeros((m, M, 2), np.float32)
        for p in range(t // M):
            u = u + (self.taps[r + p * M][None, :, None] * span[at[:, None] - (r + p * M)[None, :]])
        v = np.take_along_axis(u, ((r[None, :] + (nd % M)[:, None]) % M)[:, :, None], axis=1)
        out = fft_plus(v, self.cos, self.sin).transpose(1, 0, 2)
        self.hist = span[len(span) - (t - 1):]
        self.total += len(x)
        return np.ascontiguousarray(out[self.channels])


def chan_ref(x, n_channels, decimation, taps, cos, sin, channels=None, first_sample=0):
    """The whole stream in one call."""
    return ChanRef(n_channels, decimation, taps, cos, sin, channels, first_sample).process(x)


def channel_step(c, n_channels):
    """The DDC step of channel c's centre: c L / M, wrapped into [-32768, 32767]."""
    s = c * L // n_channels
    return s - L if s > 32767 else s


# -- the end-to-end fixture: tests/ddc_ref.py's cu8 wide stream with the carriers re-centred on channel centres, so that the
#    two bands are channels (1, 6) of 8 and (2, 12) of 16 ---------------------------------------------------------------------
E2E = dict(R.E2E, steps=(8192, -16384))
SHAPES = {8: (8, 8, (1, 6)), 16: (16, 8, (2, 12))}  # M: (M, D, channels)


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
    return synth.lowpass_taps(8, 8)
