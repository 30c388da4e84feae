"""Randomised parity over the features that came after the path fuzz (tests/test_gpu_fuzz_paths.py), drawn together: a hop
below the block size on the device and on the staged paths, 8-bit input on every delivery, windows that change or go away
in mid-stream, a first frame other than 0, sdr_attach_at, sdr_listener_stop and the control setters between the batches, and
the FFT kernel switches.  Seeded streams (tests/fuzz_features_gen.py) through the shared Case driver (tests/parity_case.py)
against the oracle, bit for bit: frame records, keying bits, edges and runes with their frames, decoder state, the exact and
the kept cumulation rows, peaks, drop counters of 0 - and with trace (every seed with a hop, every fourth dense one) the tap
values, raw and debounced bits and sampled psd and dB rows.  Every third seed is adversarial (a silent run cut inside a
hop, full-scale frames of its format); what makes it so is asserted on the oracle's own input.

The default set is fuzz_features_gen.DEFAULT_SEEDS seeds (tests/test_fuzz_features_coverage.py pins what it reaches); a
longer soak: SDR_FUZZ_FEATURES_SEEDS=300."""
import os

import numpy as np
import pytest

import fuzz_features_gen as gen
import iq8_tools
from parity_tools import capi, environment, frames_of  # noqa: F401 (capi: the fixture)

pytestmark = pytest.mark.gpu

N_SEEDS = int(os.environ.get("SDR_FUZZ_FEATURES_SEEDS", str(gen.DEFAULT_SEEDS)))


def assert_adversarial(s, case, bands):
    """The stream is what its kind says, on the oracle's own input: a case cannot quietly stop being adversarial."""
    n, hop, b = s.n, s.hop, s.adv_band
    if s.iq8 is not None:  # every byte value, as I and as Q, in the first frames of every band
        for f32, q, _ in bands:
            head = q[:iq8_tools.POOL * max(hop, 512)]
            assert len(np.unique(head[:, 0])) == 256 and len(np.unique(head[:, 1])) == 256, "not every byte value as I and as Q"
            assert np.array_equal(iq8_tools.to_f32(q, s.iq8), f32)
    if s.kind == "silent":
        a, e = s.silent_at, s.silent_at + s.silent_len
        assert a % hop != 0 and s.total - s.silent_behind >= 200
        assert not np.any(bands[b][0][a:e])
        whole = -(-a // hop)  # the first frame that starts inside the run: it ends inside it too
        assert whole * hop + n <= e and not np.any(frames_of(bands[b][0], n, hop, whole, whole + 1))
        assert np.isnan(case.outs[b]["frames"]["listen_thr"][-1]), "the silent run leaves no NaN behind"
    elif s.kind == "full_scale":
        q = bands[b][1]
        first, count, one = s.full_frames()
        fr = frames_of(q, n, hop, first, first + count)
        values, lone = {"sc16": ([32767, -32767, -32768], -32768), "cs8": ([127, -128], -128), "cu8": ([0, 255], 0)}[s.fmt]
        assert count >= 3 and np.all(np.isin(fr, values)), "frames that are not full scale"
        assert np.all(frames_of(q, n, hop, one, one + 1) == lone), f"no frame of {lone} only"
        assert len(np.unique(fr)) == len(values)


def run_seed(capi, s):
    case, bands = gen.case_of(s)
    with environment(**s.env):
        case.run(capi, min_edges=0, activity=False).close()
    assert_adversarial(s, case, bands)


@pytest.mark.parametrize("seed", range(N_SEEDS), ids=lambda seed: gen.Seed(seed).ident())
def test_random_features(capi, seed):
    run_seed(capi, gen.Seed(seed))
