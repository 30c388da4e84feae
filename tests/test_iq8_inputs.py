"""The 8-bit tests' input (tests/iq8_tools.py), checked without a GPU: a parity test between two banks proves nothing if
both see silence.  The quantised stream holds every byte value in the I and in the Q position of every frame, the oracle's
noise floor over it is finite in every frame, the oracle finds peaks in it and its listeners decode the text."""
import numpy as np
import pytest

import iq8_tools as t8
from oracle import oracle as orc


@pytest.mark.parametrize("fmt", t8.FORMATS, ids=t8.FORMAT_IDS)
def test_every_byte_value_in_i_and_q_of_every_frame(fmt):
    for n in (512, 16384):
        q, _, _ = t8.pool(n, 6, 5, fmt, oracle_psd=False)
        for p in range(t8.POOL):
            assert len(np.unique(q[p, 0::2])) == 256 and len(np.unique(q[p, 1::2])) == 256, (n, p)
    s, _ = t8.stream(2048, 512, 5, 4, 6, fmt)
    assert len(np.unique(s[:512, 0])) == 256 and len(np.unique(s[:512, 1])) == 256


def test_cu8_is_cs8_plus_128_and_the_values_are_the_contract():
    a, _, _ = t8.pool(512, 6, 7, t8.CS8, oracle_psd=False)
    b, _, _ = t8.pool(512, 6, 7, t8.CU8, oracle_psd=False)
    assert a.dtype == np.int8 and b.dtype == np.uint8
    x = np.arange(-128, 128)
    assert np.array_equal(t8.to_f32(x.astype(np.int8), t8.CS8).astype(np.float64), x / 128.0)
    u = np.arange(256)
    assert np.array_equal(t8.to_f32(u.astype(np.uint8), t8.CU8).astype(np.float64), (2.0 * u - 255.0) / 256.0)


@pytest.mark.parametrize("fmt", t8.FORMATS, ids=t8.FORMAT_IDS)
def test_the_oracle_hears_something(fmt):
    n, frames, tones = 512, 700, 6
    q, bins, _ = t8.pool(n, tones, 11, fmt, frames=frames, oracle_psd=False)
    r = orc.Receiver(t8.RATE[n], n, 70 * n // 512, 15.0, 1)
    for b in bins:
        r.attach(int(b))
    out = r.process(t8.to_f32(q, fmt))
    assert np.all(np.isfinite(out["frames"]["noise_floor"])), "the noise floor is not finite: the quantised noise is silence"
    assert out["n_chunks"] >= 6 and all(len(p) > 0 for p in out["peaks"][:out["n_chunks"]]), "a cumulation without peaks"
    assert np.count_nonzero(np.diff(out["deb"].astype(np.int8), axis=0)) > 100, "hardly any keying edges"
    texts = [r.text(lid) for lid in range(tones)]
    assert any("dl1abc" in t.lower() for t in texts), texts
