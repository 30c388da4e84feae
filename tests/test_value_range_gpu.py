"""Every stage driven with psd words across the whole float32 range, bit for bit against the oracle.

The parity tests elsewhere run at one amplitude (psd words with exponents in a band about 40 wide) plus exact zero.  Here
the same stream is placed by a power of two (tests/value_range_gen.py) so that the psd words are subnormal (low), small
multiples of 2^-149 with zeros among them (floor), zero over whole noise windows (zero_edge), just under overflow (high),
+Inf at the carriers, in part of the noise or nearly everywhere (carrier_inf, noise_inf, all_inf), or walk over 670 dB
within one cumulation (breathing).  tests/test_value_range_host.py holds the conditions that make each case what its name
says.  A receiver with its gain at either end of the float32 range is a plain finite input; these are the branches of the
device code written for it: the dB shortcut's `special`, the cumulation bound's floor_hw and unit counts, the scan's
hw_max >= 0x7f80, noise_cert's why = 1, and the FFT kernels' own float64 -> float32 store of re^2 + im^2.

What is compared: everything parity_case.Case compares (frame records, keying bits, edges, runes, text, decoder state,
exact cumulation rows, the kept row, peaks with frequencies, drop counters of 0) and, on top, the psd row and the dB
spectrum row themselves for at least 8 frames of the last batch."""
import numpy as np
import pytest

import value_range_gen as gen
from oracle import oracle as orc
from parity_case import Case
from parity_tools import bits_equal, capi, check_device_batch, environment, nan_equal_bits  # noqa: F401 (capi: the fixture)

pytestmark = pytest.mark.gpu


def mixed(regime, psd):
    """The row holds the classes the regime is about side by side (None: the regime has no such row)."""
    if regime in ("floor", "zero_edge"):
        return bool(np.any(psd == 0) and np.any(gen.subnormal(psd)))
    if regime in ("carrier_inf", "noise_inf", "all_inf"):
        return bool(np.any(np.isinf(psd)) and np.any(np.isfinite(psd)))
    return None


def check_rows(bank, case, regime, a, e):
    """psd and dB spectrum rows of the last batch [a, e) against the oracle: 8 frames spread over the batch and the first
    frame whose row mixes the regime's classes."""
    frames = sorted({int(x) for x in np.linspace(0, e - a - 1, 8)})
    for b in range(case.n_bands):
        host = case.oracle_input(b)
        want = {f: orc.iq_to_spectrum_and_psd(host[a + f]) for f in frames}
        if mixed(regime, want[frames[0]][1]) is not None and not any(mixed(regime, w[1]) for w in want.values()):
            for f in range(e - a):
                w = orc.iq_to_spectrum_and_psd(host[a + f])
                if mixed(regime, w[1]):
                    want[f] = w
                    break
            else:
                raise AssertionError(f"band {b}: no frame of the last batch mixes the classes of {regime}")
        assert len(want) >= 8
        for f, (want_sp, want_psd) in sorted(want.items()):
            sp, psd = bank.read_spectrum(b, f)
            assert nan_equal_bits(psd, want_psd), f"band {b} frame {a + f} psd: {np.flatnonzero(psd.view(np.uint32) != want_psd.view(np.uint32))[:8]}"
            assert nan_equal_bits(sp, want_sp), f"band {b} frame {a + f} spectrum"


def make_case(spec):
    bands = spec.bands()
    return Case(spec.n, spec.n_bands, None, 0, [("batch", x) for x in spec.batches], seed=spec.seed(), rate=gen.RATES[spec.n],
                path=spec.path, bands=bands, init_bins=[gen.listeners(spec.n, bd[2]) for bd in bands], nan_ok=spec.regime in gen.NAN_OK)


@pytest.mark.parametrize("spec", gen.MATRIX, ids=[s.id for s in gen.MATRIX])
def test_value_range(capi, spec):
    case = make_case(spec)
    with environment(**dict(spec.env)):
        bank = case.run(capi, min_edges=0, activity=spec.regime in gen.ACTIVE)
    check_rows(bank, case, spec.regime, spec.frames - spec.batches[-1], spec.frames)
    bank.close()


class VCase(Case):
    """Dense frames of one band on a bank with trace, reading back at least 8 rows of every batch that has as many."""

    def spectrum_frames(self, frames):
        return sorted(set(super().spectrum_frames(frames)) | {int(x) for x in np.linspace(0, frames - 1, 8)})


@pytest.mark.parametrize("spec", gen.WINDOWED, ids=[s.id for s in gen.WINDOWED])
def test_value_range_windowed(capi, spec):
    """The windowed code objects have an input step of their own: float32 samples and table each carrying half of the
    exponent, and int16 samples whose table carries all of it (the only way the sc16 kernels reach these levels)."""
    s, q, w, carriers = gen.windowed_input(spec)
    run = VCase(spec.n, 1, None, 0, [("batch", x) for x in spec.batches], seed=0, rate=gen.RATES[spec.n],
                path="device_sc16" if spec.sc16 else "device", bands=[(s, q, carriers)], init_bins=[gen.listeners(spec.n, carriers)],
                windows=[w] * len(spec.batches), trace=True)
    assert len(run.spectrum_frames(spec.batches[-1])) >= 8
    edges, peaks = run.oracle_counts()
    if spec.regime in gen.ACTIVE:
        assert edges > 0 and peaks > 0
    run.run(capi, min_edges=0, activity=spec.regime in gen.ACTIVE).close()


# -- non-finite samples -------------------------------------------------------------------------------------------------
# DESIGN 3, "Inf / NaN inputs": one sample component of ONE frame of band 0 is +Inf, -Inf or NaN.  The reference carries
# out every multiplication, also those by the twiddles 1 and -i: (Inf + bi)(1 + 0i) = (Inf, NaN).  k_fft_psd and k_fft_r32
# skip them and keep (Inf, b).  tests/emu (emu_fft, emu_fft_r32, emu_fft_2p with the argument `nonfinite`;
# test_value_range_host.py pins the table) found: every psd word of the frame is non-finite on both sides; an infinite
# sample at index N/4, N/2 or 3N/4 gives a row of NaN in the reference and of +Inf in those two kernels; every other case,
# and every case of k_fft_2p, gives the same class in every word.
POISONED = 37  # the frame, inside the first cumulation
VALUES = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan}
POSITIONS = {"0": lambda n: 0, "N/4": lambda n: n // 4, "N/2": lambda n: n // 2, "3N/4": lambda n: 3 * n // 4, "odd": lambda n: n // 4 + 37}
TABLE = [(v, p, at) for v in VALUES for p in (0, 1) for at in POSITIONS]  # every case of tests/emu's table, on every bank
NON_FINITE = (
    [("psd9", 512, (1, 70, 130, 59), (), v, p, at) for v, p, at in TABLE]
    + [("r32", 16384, (1024, 76), (), v, p, at) for v, p, at in TABLE]  # (the frame is in the launch of 1024)
    + [("2p32768", 32768, gen.SHORT, gen.GROUPS, v, p, at) for v, p, at in TABLE]
)
THRESHOLDS = ("noise_floor", "noise_dev", "peak_thr", "listen_thr")
PER_FRAME = ("min_mean", "variance", "dev_in", "nf_in")  # of one frame's psd alone: the frames around the poisoned one keep theirs


def classes_differ(kernel, value, at):
    """tests/emu's table: where the bank's row is +Inf and the reference's NaN."""
    return kernel != "2p32768" and value != "nan" and at in ("N/4", "N/2", "3N/4")


class PoisonedCase(Case):
    """Band 0 holds the poisoned frame, band 1 is an ordinary band.  What sdr_poll delivers (edges, runes, peaks of both
    bands), text, decoder state and drop counters are compared as in every Case: equal to the oracle's.  What stays on the
    device is compared here: band 1 bit for bit, band 0 as far as the statement goes."""

    differ = False

    def check_device(self, bank, a, e, k, cumulations=True):
        P = POISONED
        check_device_batch(_OneBand(bank, 1), [self.outs[1]], a, e, 1, [self.live(1, a, e)], k)
        out = self.outs[0]
        recs, want = bank.read_frame_records(0), out["frames"][a:e]
        at = np.arange(a, e)
        for f in PER_FRAME:
            assert bits_equal(recs[f][at != P], want[f][at != P].copy()), f"band 0 batch {k} field {f} beside the poisoned frame"
        for f in THRESHOLDS:
            assert bits_equal(recs[f][at < P], want[f][at < P].copy()), f"band 0 batch {k} field {f} before the poisoned frame"
            assert not np.any(np.isfinite(recs[f][at >= P])) and not np.any(np.isfinite(want[f][at >= P])), f"band 0 field {f}: finite behind the poisoned frame"
            assert np.all(np.isnan(recs[f][at >= P + 60])) and np.all(np.isnan(want[f][at >= P + 60])), f"band 0 field {f}: not NaN 60 frames on"
        for lid in self.live(0, a, e):
            assert np.array_equal(bank.read_keying_bits(0, lid), out["deb"][a:e, lid]), f"band 0 listener {lid} batch {k}"
        for c in range(bank.last_batch_chunks):
            pk, _, fr = bank.read_peaks(0, c)
            gc = list(out["peak_frames"]).index(a + fr)
            got, exact = bank.read_cumulation(0, c), out["cumulation"][gc]
            assert pk == out["peaks"][gc]
            if gc == P // 100:
                assert not np.any(np.isfinite(got)) and not np.any(np.isfinite(exact)), "the poisoned cumulation holds a finite bin"
                assert pk == []
            else:
                assert bits_equal(got, exact), f"band 0 cumulation {gc}"
        if a <= P < e:
            self.saw_frame = True
            for f in ({P - 1, P + 1} & set(range(a, e))) | {P}:
                sp, psd = bank.read_spectrum(0, f - a)
                want_sp, want_psd = orc.iq_to_spectrum_and_psd(self.frames(0, f, f + 1))
                if f != P:
                    assert bits_equal(psd, want_psd) and bits_equal(sp, want_sp), f"band 0 frame {f}: the poisoned frame's neighbour"
                    continue
                assert not np.any(np.isfinite(psd)) and not np.any(np.isfinite(want_psd))
                assert not np.any(np.isfinite(recs["min_mean"][P - a])) and not np.any(np.isfinite(want["min_mean"][P - a]))
                if self.differ:
                    assert np.all(np.isposinf(psd)) and np.all(np.isnan(want_psd)), "the documented difference is gone: correct DESIGN 3"
                else:
                    assert nan_equal_bits(psd, want_psd) and nan_equal_bits(sp, want_sp)
            sp, psd = bank.read_spectrum(1, P - a)
            want_sp, want_psd = orc.iq_to_spectrum_and_psd(self.frames(1, P, P + 1))
            assert bits_equal(psd, want_psd) and bits_equal(sp, want_sp), "band 1 at the poisoned frame"


class _OneBand:
    """A bank seen as its band `band` alone (band 0 of the view), for check_device_batch."""

    def __init__(self, bank, band):
        self._bank, self._band = bank, band

    def __getattr__(self, name):
        f = getattr(self._bank, name)
        if name.startswith("read_"):
            return lambda b, *a: f(self._band, *a)
        return f


@pytest.mark.parametrize("kernel, n, batches, env, value, part, at", NON_FINITE,
                         ids=[f"{k}-{v}-{('re', 'im')[p]}-{at.replace('/', '_')}" for k, _, _, _, v, p, at in NON_FINITE])
def test_non_finite_sample_poisons_its_band_only(capi, kernel, n, batches, env, value, part, at):
    frames = sum(batches)
    assert frames >= 230  # (the rolling means pass the 60-frame mark behind POISONED and a second cumulation completes)
    bands = []
    for b in range(2):
        iq, bins = gen.base(n, frames, 9700 + n // 64 + 17 * b)
        bands.append((iq.copy(), None, bins))  # (the generator's array is shared and read-only)
    bands[0][0][POISONED, 2 * POSITIONS[at](n) + part] = VALUES[value]
    case = PoisonedCase(n, 2, None, 0, [("batch", x) for x in batches], seed=0, rate=gen.RATES[n], bands=bands,
                        init_bins=[gen.listeners(n, bd[2]) for bd in bands], nan_ok=True)
    case.differ, case.saw_frame = classes_differ(kernel, value, at), False
    with environment(**dict(env)):
        bank = case.run(capi, min_edges=0, activity=False)
    assert case.saw_frame
    out = case.outs[1]  # the ordinary band is alive: it keys, finds peaks in both cumulations and decodes
    assert np.count_nonzero(np.diff(out["deb"].astype(np.int8), axis=0)) > 0 and all(len(p) > 0 for p in out["peaks"][:2])
    assert np.all(np.isfinite(out["frames"]["listen_thr"]))
    bank.close()
