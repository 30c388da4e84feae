"""What keeps tests/test_value_range_gpu.py honest, on the CPU: every (regime, block size) it runs is what its name says on
the ORACLE's numbers - these are conditions the generator (tests/value_range_gen.py) has to meet, not measurements - and
the oracle's own rounding at these levels is what numpy's is: a stream times 2^k has the FFT times 2^k exactly, and a psd
word is float32(re * re + im * im) with numpy's cast, subnormals and +Inf included."""
import functools

import numpy as np
import pytest

import value_range_gen as gen
from oracle import oracle as orc
from sdrainer_amd import synth


class Oracle:
    """One band through the oracle: the run's output, the psd rows of frames 0, 13, 26 ... and what they are made of."""

    def __init__(self, n, frames_in, bins, edge=None):
        self.n, self.bins, self.iq = n, bins, frames_in
        self.edge = synth.default_edge_width(n) if edge is None else edge
        r = orc.Receiver(gen.RATES[n], n, self.edge)
        for b in gen.listeners(n, bins):
            r.attach(int(b))
        self.out = r.process(frames_in, max_peaks=4096)
        self.at = list(range(0, frames_in.shape[0], gen.SAMPLED))
        self.psd = np.stack([orc.iq_to_spectrum_and_psd(frames_in[f])[1] for f in self.at])
        self.noise = gen.noise_mask(n, bins)
        self.rec = self.out["frames"]

    def thresholds_finite(self):
        return all(np.all(np.isfinite(self.rec[f])) for f in ("noise_floor", "noise_dev", "peak_thr", "listen_thr"))

    def windows(self, row):
        w = (self.n - 2 * self.edge) // 10
        return [row[self.edge + k * w:self.edge + (k + 1) * w] for k in range(10)]

    def edges(self):
        return int(np.count_nonzero(np.diff(self.out["deb"].astype(np.int8), axis=0)))


def check_regime(regime, o):
    """The regime's conditions on one band's oracle run."""
    psd, rec, out = o.psd, o.rec, o.out
    assert not np.any(np.isnan(psd)) and not np.any(psd < 0)
    if regime == "low":
        assert np.mean(gen.subnormal(psd)) >= 0.90
        assert o.thresholds_finite()
        assert len(out["peaks"]) >= 2 and all(len(p) >= 1 for p in out["peaks"])
        assert o.edges() >= 1
    elif regime == "floor":
        assert 0.03 <= np.mean(psd == 0) <= 0.40
        assert np.all(gen.subnormal(psd[psd != 0]))
        assert o.thresholds_finite()
        assert np.any((psd[:, 1:] == psd[:, :-1]) & (psd[:, 1:] != 0))
    elif regime == "zero_edge":
        at = np.flatnonzero(rec["min_mean"] == 0)
        assert len(at) >= 1
        assert any(np.any(orc.iq_to_spectrum_and_psd(o.iq[f])[1]) for f in at[:8])
    elif regime == "high":
        assert np.all(np.isfinite(psd)) and np.all(np.isfinite(out["cumulation"]))
        assert psd.max() >= np.float32(2.0 ** 124)
        assert o.thresholds_finite()
    elif regime == "carrier_inf":
        assert np.any(np.isinf(psd)) and not np.any(np.isinf(psd[:, o.noise]))
        every = np.stack([orc.iq_to_spectrum_and_psd(x)[1] for x in o.iq])  # (all frames: a carrier is keyed about a third of the time)
        assert not np.any(np.isinf(every[:, o.noise]))
        for k in range(10):  # every noise window: free of Inf in at least half of the frames
            assert np.mean([not np.any(np.isinf(o.windows(row)[k])) for row in every]) >= 0.5, f"window {k}"
        assert len(out["peaks"]) >= 2 and all(len(p) >= 1 for p in out["peaks"])
    elif regime == "noise_inf":
        assert 0.01 <= np.mean(np.isinf(psd[:, o.noise])) <= 0.60
    elif regime == "all_inf":
        assert np.any(np.isposinf(rec["min_mean"]) & np.isnan(rec["variance"]))
    else:
        assert regime == "breathing"
        assert all(np.all(np.isfinite(rec[f])) for f in rec.dtype.names)
        assert np.all(np.isfinite(out["cumulation"])) and np.all(psd > 0) and np.all(np.isfinite(psd))
        assert len(out["peaks"]) >= 2 and all(len(p) >= 1 for p in out["peaks"])  # (not the issue's: the GPU case asks for activity)
        for c in range(2):
            nf = rec["nf_in"][100 * c:100 * (c + 1)].astype(np.float64)
            assert nf.max() - nf.min() >= 600.0, f"cumulation {c}: {nf.max() - nf.min():.1f} dB"


@functools.lru_cache(maxsize=None)
def spec_checked(spec):
    for iq, _, bins in spec.bands():
        check_regime(spec.regime, Oracle(spec.n, iq, bins))
    return True


def check_batches(batches):
    """At least 230 frames, a batch of 1, one of fewer than 100 frames and one across a cumulation boundary."""
    assert sum(batches) >= 230 and 1 in batches and any(1 < x < 100 for x in batches)
    pos, crosses = 0, False
    for x in batches:
        crosses |= (pos + x - 1) // 100 > pos // 100 and pos % 100 != 0
        pos += x
    assert crosses, "no batch across a cumulation boundary"


# ordered by stream, so that value_range_gen.base's cache serves the regimes of one geometry
@pytest.mark.parametrize("spec", gen.MATRIX, ids=[s.id for s in gen.MATRIX])
def test_regime_is_what_its_name_says(spec):
    check_batches(spec.batches)
    assert spec_checked(spec)


def test_every_case_picks_the_kernels_its_id_names(tmp_path):
    """The library's own batch plan (tests/host/fuzz_paths_plan.cpp) for every batch of every case: the FFT kernel, the
    wide tap and the noise path are the id's, so that a moved threshold cannot quietly empty a row of the matrix."""
    import os
    import subprocess
    host = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host")
    exe = str(tmp_path / "fuzz_paths_plan")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(host, "fuzz_paths_plan.cpp")])
    lines, rows = [], []
    for spec in gen.MATRIX:
        slots, pos = len(gen.listeners(spec.n, gen.base(spec.n, spec.frames, spec.seed())[1])), 0
        for x in spec.batches:
            lines.append(f"{spec.n} {spec.n_bands} {max(spec.batches)} {x} {pos % 100} 0 {slots}")
            rows.append((spec, x))
            pos += x
    run = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr
    names = ("r32", "wide_tap", "two_phase", "group_frames", "scan_parts", "gather_peaks", "noise_scan", "bound")
    plans = [dict(zip(names, (int(v) for v in ln.split()))) for ln in run.stdout.split("\n") if ln]
    assert len(plans) == len(rows)
    for (spec, x), plan in zip(rows, plans):
        want = dict(gen.PLAN[spec.kernel])
        if spec.kernel == "r32" and x < 1024:  # (the short batches around the launch: k_fft_psd<14>, no wide tap)
            want.update(r32=0, wide_tap=0)
        assert {k: plan[k] for k in want} == want, (spec.id, x, plan)
        if plan["two_phase"]:  # the case's own frame groups: the batch of 120 spans several
            mib = int(dict(spec.env)["SDR_FFT2P_GROUP_MB"])
            assert max(spec.batches) > (mib << 20) // (spec.n_bands * spec.n * 16)


@pytest.mark.parametrize("spec", gen.WINDOWED, ids=[s.id for s in gen.WINDOWED])
def test_windowed_regime_is_what_its_name_says(spec):
    check_batches(spec.batches)
    s, q, w, bins = gen.windowed_input(spec)
    n = spec.n
    if spec.sc16:
        assert np.array_equal(s.reshape(-1), q.reshape(-1).astype(np.float32) / np.float32(32767.0))
        assert np.abs(s).max() > 0.5  # the samples carry no part of the exponent
    else:
        assert 2.0 ** -45 < np.abs(s).max() < 2.0 ** -25 and 2.0 ** -45 < w.max() < 2.0 ** -25  # half each
    frames = (s.reshape(-1, n, 2) * w[None, :, None]).astype(np.float32).reshape(-1, 2 * n)
    check_regime(spec.regime, Oracle(n, frames, bins))


UNIFORM = [s for s in gen.MATRIX if s.kernel in ("psd9", "psd13") and s.regime != "breathing"]


@pytest.mark.parametrize("spec", UNIFORM, ids=[s.id for s in UNIFORM])
def test_oracle_fft_scales_exactly_and_psd_rounds_as_numpy(spec):
    x, _ = gen.base(spec.n, spec.frames, spec.seed())
    k = gen.exponents(spec.regime, spec.n, spec.frames, spec.seed())
    classes = set()
    for f in range(0, spec.frames, 4 * gen.SAMPLED):
        xs = gen.scale(x[f], k)
        assert np.array_equal(xs.astype(np.float64), np.ldexp(x[f].astype(np.float64), k)), "the scaling is not exact"
        X, Xs = orc.iq_fft(x[f]), orc.iq_fft(xs)
        assert np.array_equal(Xs.real, np.ldexp(X.real, k)) and np.array_equal(Xs.imag, np.ldexp(X.imag, k)), f"frame {f}"
        with np.errstate(over="ignore", under="ignore"):
            want = np.roll((Xs.real * Xs.real + Xs.imag * Xs.imag).astype(np.float32), spec.n // 2)  # (spectrum order)
        _, psd = orc.iq_to_spectrum_and_psd(xs)
        assert np.array_equal(psd.view(np.uint32), want.view(np.uint32)), f"frame {f}: psd words"
        classes |= {"zero"} if np.any(psd == 0) else set()
        classes |= {"subnormal"} if np.any(gen.subnormal(psd)) else set()
        classes |= {"inf"} if np.any(np.isinf(psd)) else set()
    need = {"low": {"subnormal"}, "floor": {"zero", "subnormal"}, "zero_edge": {"zero", "subnormal"}, "high": set(),
            "carrier_inf": {"inf"}, "noise_inf": {"inf"}, "all_inf": {"inf"}}[spec.regime]
    assert need <= classes, (need, classes)


# -- non-finite samples ("Inf / NaN inputs") -------------------------------------------------------------------
EMUS = {"emu_fft": (512, 16384), "emu_fft_r32": (16384,), "emu_fft_2p": (32768, 65536)}


@pytest.mark.parametrize("emu", EMUS)
def test_non_finite_sample_classes_on_the_cpu(tmp_path, emu):
    """One sample component +Inf, -Inf or NaN, in re or im, at sample 0, N/4, N/2, 3N/4 and an odd index, through the
    kernels' own phase functions on the CPU (tests/emu, argument `nonfinite`) and through the oracle: the statement of
    DESIGN 3 that tests/test_value_range_gpu.py::test_non_finite_sample_poisons_its_band_only then holds the bank to.
    Every psd word of such a frame is non-finite on both sides and all words of a row have one class.  The reference
    multiplies by the twiddles 1 and -i, (Inf + bi)(1 + 0i) = (Inf, NaN); k_fft_psd and k_fft_r32 skip those
    multiplications: an infinite sample at N/4, N/2 or 3N/4 gives NaN in the reference and +Inf in those kernels.  Every
    other case is the same class in both, and k_fft_2p has the reference's class everywhere."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / emu)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(root, "tests", "emu", emu + ".cpp"), "-ldl"])
    out = subprocess.run([exe, orc.build(), "nonfinite"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("nonfinite ")]
    assert len(rows) == 30 * len(EMUS[emu])
    for r in rows:  # nonfinite N=<n> <value> <re|im> @<index>: kernel <finite> <inf> <nan> oracle <finite> <inf> <nan>
        n, value, at = int(r[1][2:]), r[2], int(r[4][1:-1])
        kernel, oracle = tuple(int(x) for x in r[6:9]), tuple(int(x) for x in r[10:13])
        inf_row, nan_row = (0, n, 0), (0, 0, n)
        if value == "nan" or at % (n // 4):
            assert kernel == oracle == nan_row, r
        elif at == 0:
            assert kernel == oracle == inf_row, r
        else:
            assert oracle == nan_row and kernel == (nan_row if emu == "emu_fft_2p" else inf_row), r
