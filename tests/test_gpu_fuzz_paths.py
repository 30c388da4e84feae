"""Randomised parity over every FFT kernel, input path and band count: seeded streams (tests/fuzz_paths_gen.py) through
the shared Case driver (tests/parity_case.py) against the oracle, bit for bit - frame records, keying bits, edges and
runes as sdr_poll delivers them, decoder state, the exact cumulation rows and the kept row, peaks with their
frequencies, drop counters of 0.  Every second seed holds adversarial frames (silent runs, exactly tied noise windows,
exactly tied peak bins, full-scale int16), and each kind also runs as a named case at every block size.

The default set is fuzz_paths_gen.DEFAULT_SEEDS seeds (tests/test_fuzz_paths_coverage.py pins what it reaches); a longer
soak: SDR_FUZZ_PATHS_SEEDS=200.  test_gpu_fuzz.py's seeds are older history and stay as they are."""
import os

import numpy as np
import pytest

import fuzz_paths_gen as gen
from oracle import oracle as orc
from parity_case import Case
from parity_tools import capi  # noqa: F401 (the fixture)

pytestmark = pytest.mark.gpu

N_SEEDS = int(os.environ.get("SDR_FUZZ_PATHS_SEEDS", str(gen.DEFAULT_SEEDS)))


def _assert_adversarial(s, case, bands):
    """The frames are what their kind says, on the oracle's own numbers: the case cannot quietly stop being adversarial."""
    n, b = s.n, s.adv_band
    if s.kind == "tied_windows":
        edge, w = gen.tied_window(n)
        assert case.edge == edge and (n - 2 * edge) % 10 == 0 and n % w == 0
        for f in s.tied_frames[:8]:
            _, psd = orc.iq_to_spectrum_and_psd(bands[b][0][f])
            x = psd.astype(np.float64)
            sums = [sum(x[edge + k * w:edge + (k + 1) * w].tolist()) for k in range(9)]  # (dsp/fft.go:239-241: in order)
            assert len(set(sums)) == 1 and sums[0] > 0, f"frame {f}: the window sums are not tied"
    elif s.kind == "tied_peaks":
        out = case.outs[0]
        assert len(out["peaks"]) >= 2
        for cum, peaks in zip(out["cumulation"], out["peaks"]):
            assert len(peaks) == n // 4
            for p in peaks:
                sb = p[6]
                assert p[0] <= sb < p[1] and cum[sb] == cum[sb + 1] and cum[sb].tobytes() == cum[sb + 1].tobytes(), p
    elif s.kind == "silent":
        thr = case.outs[b]["frames"]["listen_thr"]
        assert np.isnan(thr[-1]) and s.total - (s.silent_at + s.silent_len) >= 200
        assert not np.any(bands[b][0][s.silent_at:s.silent_at + s.silent_len])
    elif s.kind == "full_scale":
        q = bands[b][1]
        full = np.all(np.isin(q, [32767, -32767, -32768]), axis=1)
        assert full.sum() >= 3 and np.any(np.all(q == -32768, axis=1))


def run_seed(capi, s):
    bands = s.inputs()
    steps, init = s.steps([bd[2] for bd in bands])
    case = Case(s.n, s.n_bands, None, 0, steps, seed=s.seed, rate=s.rate, edge=s.edge, debounce=s.debounce,
                threshold=[bd["threshold"] for bd in s.bands], centers=[bd["center"] for bd in s.bands], path=s.path, bands=bands,
                init_bins=init, max_peaks=max(1024, s.n // 4 + 16) if s.kind == "tied_peaks" else 1024, nan_ok=s.kind == "silent")
    case.run(capi, min_edges=0, activity=False).close()
    _assert_adversarial(s, case, bands)


def _id(seed):
    s = gen.Seed(seed)
    return f"seed{seed:03d}-{s.n}-{s.path}-{s.n_bands}b-{s.kind}"


@pytest.mark.parametrize("seed", range(N_SEEDS), ids=_id)
def test_random_paths(capi, seed):
    run_seed(capi, gen.Seed(seed))


# the named adversarial cases: every kind at every block size, through a float32 and an int16 path by turns
NAMED = [(kind, n, path) for i, n in enumerate(gen.SIZES) for kind, path in (
    ("silent", ("device", "kiwi")[i % 2]), ("tied_windows", ("staged", "device_sc16")[i % 2]),
    ("tied_peaks", ("device", "staged")[i % 2]), ("full_scale", ("staged_sc16", "device_sc16")[i % 2]))]


@pytest.mark.parametrize("kind, n, path", NAMED, ids=[f"{k}-{n}-{p}" for k, n, p in NAMED])
def test_adversarial_frames(capi, kind, n, path):
    run_seed(capi, gen.Seed(5000 + gen.SIZES.index(n), n=n, path=path, kind=kind))
