"""The IQ correction and the raw stream's sums restated in NumPy (include/sdrainer_hip.h "IQ correction"): the oracle of
tests/test_iqc_ref.py and test_iqc_gpu.py.  correct() is the four float32 operations of the contract, one per line; sums()
is int64; from_sums() is the float64 sequence, one operation per line.  A corrected stream is tests/ddc_ref.py or
tests/chan_ref.py fed correct()'s values; CorrectedDdcRef keeps the RAW carry, so that a change of the correction between
two calls is modelled.  The impaired end-to-end fixture is here too.  A plain helper module, not a test file."""
import numpy as np

import ddc_ref as R
from sdrainer_amd import synth

SCALE = {R.CS8: 128.0, R.CU8: 256.0, R.SC16: 32767.0}
SUM_FORMATS = (R.CS8, R.CU8, R.SC16)
SUM_FORMAT_IDS = ("cs8", "cu8", "sc16")
FIELDS = ("n", "sum_i", "sum_q", "sum_ii", "sum_qq", "sum_iq", "skipped", "reserved")


def correct(x, corr):
    """x [n, 2] float32 (what the format makes of the raw words), corr None or (dc_re, dc_im, gain_im, cross)."""
    x = np.asarray(x, np.float32).reshape(-1, 2)
    if corr is None:
        return x
    dc_re, dc_im, gain_im, cross = (np.float32(v) for v in corr)
    re1 = x[:, 0] - dc_re
    im1 = x[:, 1] - dc_im
    im = (gain_im * im1) + (cross * re1)
    return np.stack([re1, im], axis=1)


def units(raw, fmt):
    """The integer units of raw samples [n, 2], int64: cs8 x, cu8 2 x - 255, sc16 x."""
    u = np.asarray(raw, R.RAW_DTYPE[fmt]).astype(np.int64)
    return 2 * u - 255 if fmt == R.CU8 else u


def sums(raw, fmt):
    u = units(raw, fmt).reshape(-1, 2)
    i, q = u[:, 0], u[:, 1]
    return dict(n=len(u), sum_i=int(i.sum()), sum_q=int(q.sum()), sum_ii=int((i * i).sum()), sum_qq=int((q * q).sum()),
                sum_iq=int((i * q).sum()), skipped=0, reserved=0)


def add_sums(a, b):
    return {f: a[f] + b[f] for f in FIELDS}


def from_sums(s, fmt):
    """(dc_re, dc_im, gain_im, cross) as float32, or None where sdr_iq_correction_from_sums refuses."""
    if fmt not in SCALE or s["n"] < 2:
        return None
    f = np.float64
    with np.errstate(all="ignore"):
        N = f(s["n"])
        mi = f(s["sum_i"]) / N
        mq = f(s["sum_q"]) / N
        vi = f(s["sum_ii"]) / N - mi * mi
        vq = f(s["sum_qq"]) / N - mq * mq
        c = f(s["sum_iq"]) / N - mi * mq
        if not vi > 0:
            return None
        r = vq - (c * c) / vi
        if not r > 0:
            return None
        g = np.sqrt(vi / r)
        x = -(g * (c / vi))
        S = f(SCALE[fmt])
        out = (mi / S, mq / S, g, x)
        if not all(np.isfinite(v) for v in out):
            return None
        return tuple(np.float32(v) for v in out)


class CorrectedDdcRef:
    """A DDC that keeps the last T - 1 RAW samples (float32 values of the raw words) and converts them again with the
    correction current in each call: process(x, corr) with x the call's uncorrected float32 samples [n, 2]."""

    def __init__(self, decimation, taps, steps, cos, sin, first_sample=0):
        self.args = (decimation, taps, steps, cos, sin)
        self.t = len(taps)
        self.total = int(first_sample)
        self.raw = np.zeros((0, 2), np.float32)  # the carried raw samples that exist (none below the first sample)

    def process(self, x, corr):
        x = np.asarray(x, np.float32).reshape(-1, 2)
        ref = R.DdcRef(*self.args, first_sample=self.total)
        have = np.concatenate([self.raw, x])
        carried = correct(self.raw, corr)
        ref.hist[len(ref.hist) - len(carried):] = carried  # (samples below the first sample stay +0)
        out = ref.process(correct(x, corr))
        self.raw = have[max(0, len(have) - (self.t - 1)):]
        self.total += len(x)
        return out


# -- the impaired end-to-end fixture: tests/ddc_ref.py's E2E with three bands, the third empty, so that band 0's image falls
#    into band 1 and band 1's into band 0, and the DC offset into band 2 ----------------------------------------------------------
E2E = dict(R.E2E, steps=(9000, -9000, 0), bins=(320, 300), gain=1.05, phase=np.deg2rad(3.0), dc=(0.01, -0.02))
GHOST_BINS = (212, 192, 256)  # band 0: w1aw's image; band 1: dl1abc's image; band 2: the DC line


LISTEN = ((320,), (300, 192), (256,))  # listeners per band: the stations, the ghost bin of band 1, the DC line's bin
_e2e = {}


def e2e_centers():
    return [14_000_000 + int(round(s * E2E["wide_rate"] / R.L)) for s in E2E["steps"]]


def e2e_reference(table, corrected):
    """The fixture through the reference DDC and the oracle receiver, computed once per process: a dict with the raw stream,
    the narrow length, the correction (from_sums of the whole stream's sums, or None), the reference's narrow streams and the
    oracle's outputs and hop-timed decoders per band."""
    if corrected not in _e2e:
        from parity_tools import run_oracle

        e = E2E
        raw, narrow = e2e_wide()
        corr = from_sums(sums(raw, R.CU8), R.CU8) if corrected else None
        ref = R.ddc_ref(correct(R.to_f32(raw, R.CU8), corr), e["decimation"], R.e2e_taps(), e["steps"], *table)
        _, outs, decs = run_oracle(e["rate"], e["n"], e["edge"], [list(b) for b in LISTEN], list(ref), e2e_centers(), e["hop"])
        _e2e[corrected] = dict(raw=raw, narrow=narrow, corr=corr, ref=ref, outs=outs, decs=decs)
    return _e2e[corrected]


def peaks_near(out, bin_, within):
    """The cumulations of one band's oracle output that list a peak whose signal bin lies within `within` bins of bin_."""
    return sum(any(abs(p[6] - bin_) <= within for p in pk) for pk in out["peaks"])


def e2e_wide(impaired=True):
    """(cu8 [samples, 2], narrow samples per band): "dl1abc" on bin 320 of band 0, "w1aw" on bin 300 of band 1."""
    e = E2E
    narrow = (e["frames"] - 1) * e["hop"] + e["n"]
    narrow += -narrow % 4
    wide = narrow * e["decimation"]
    carriers = []
    for step, bin_, text, dit in zip(e["steps"], e["bins"], e["texts"], e["dit_ticks"]):
        offset = step * e["wide_rate"] / R.L + (bin_ - e["n"] // 2) * e["rate"] / e["n"]
        per_tick = e["hop"] * e["decimation"]
        key = np.repeat(np.concatenate([np.zeros(40, np.uint8), synth.keying_pattern(text, dit)]), per_tick)
        carriers.append((offset, e["amplitude"], key))
    x = synth.wide_stream(wide, e["wide_rate"], carriers, noise_sigma=e["sigma"], seed=e["seed"])
    if impaired:
        x = synth.impair_iq(x, e["gain"], e["phase"], e["dc"])
    return synth.quantise_iq(x, "cu8"), narrow
