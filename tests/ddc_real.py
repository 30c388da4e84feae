"""The down-converter's real input formats (include/sdrainer_hip.h SDR_DDC_REAL) for the tests: the format table, raw
streams, and the end-to-end fixture of tests/test_ddc_real_ref.py and tests/test_ddc_real_gpu.py.  A real sample v is the
complex sample (v, +0.0f), so tests/ddc_ref.py fed as_complex(v) is the oracle: nothing of the arithmetic is restated
here.  A plain helper module, not a test file."""
import numpy as np

import ddc_ref as R
from sdrainer_amd import synth

REAL = 16
RF32, RS16, RS8, RU8 = (REAL | f for f in R.FORMATS)
FORMATS = (RF32, RS16, RS8, RU8)
FORMAT_IDS = ("rf32", "rs16", "rs8", "ru8")
BASE = {f: f & ~REAL for f in FORMATS}  # the complex format of the same sample type
RAW_DTYPE = {f: R.RAW_DTYPE[BASE[f]] for f in FORMATS}


def to_f32_real(raw, fmt):
    """The float32 values of raw real samples [n]: what the complex format of the same sample type gives each word."""
    raw = np.asarray(raw, RAW_DTYPE[fmt])
    assert raw.ndim == 1
    return R.to_f32(raw, BASE[fmt])


def as_complex(v):
    """float32 [n] -> float32 [n, 2], every imaginary part +0.0."""
    v = np.asarray(v, np.float32)
    return np.stack([v, np.zeros_like(v)], axis=1)


def random_raw_real(n, fmt, seed):
    """n raw samples [n] over the format's whole range (float32: uniform in [-1, 1)); both ends of an integer range are
    present from n = 2 on, and every one of a byte format's 256 values from n = 256 on."""
    rng = np.random.default_rng(seed)
    if fmt == RF32:
        return (rng.random(n, dtype=np.float32) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    info = np.iinfo(RAW_DTYPE[fmt])
    raw = rng.integers(info.min, info.max + 1, n)
    must = np.arange(info.min, info.max + 1) if info.max - info.min < 256 else np.array([info.min, info.max])
    if n >= len(must):
        raw[rng.permutation(n)[:len(must)]] = must
    return raw.astype(RAW_DTYPE[fmt])


# -- the end-to-end fixture: one real wide stream as a direct-sampling receiver delivers it, two keyed call signs; the third
#    band tunes to the first band's carrier with the negated step and sees it mirrored, at bin N - 320 ---------------------------
E2E_REAL = dict(wide_rate=384_000, decimation=8, taps_per_phase=8, n=512, hop=128, rate=48_000, edge=70, steps=(9000, 20000, -9000),
                bins=(320, 224, 192), texts=("dl1abc dl1abc", "w1aw w1aw w1aw"), calls=("dl1abc", "w1aw", "dl1abc"),
                dit_ticks=(8, 10), idle_ticks=40, amplitude=0.4, sigma=0.02, frames=1800, seed=77)
QUANTISED = {"s16": RS16, "u8": RU8}


def e2e_real_wide(quantise):
    """(raw [samples] as `quantise` gives it, narrow samples per band): the carriers sit on bins E2E_REAL["bins"] of their
    bands' N-point spectra."""
    e = E2E_REAL
    narrow = (e["frames"] - 1) * e["hop"] + e["n"]
    narrow += -narrow % 4
    wide = narrow * e["decimation"]
    carriers = []
    for step, bin_, text, dit in zip(e["steps"], e["bins"], e["texts"], e["dit_ticks"]):
        f = step * e["wide_rate"] / R.L + (bin_ - e["n"] // 2) * e["rate"] / e["n"]
        assert 0 < f < e["wide_rate"] / 2
        per_tick = e["hop"] * e["decimation"]
        key = np.repeat(np.concatenate([np.zeros(e["idle_ticks"], np.uint8), synth.keying_pattern(text, dit)]), per_tick)
        carriers.append((f, e["amplitude"], key))
    return synth.wide_stream_real(wide, e["wide_rate"], carriers, noise_sigma=e["sigma"], seed=e["seed"], quantise=quantise), narrow


def e2e_real_taps():
    return synth.lowpass_taps(E2E_REAL["decimation"], E2E_REAL["taps_per_phase"])
