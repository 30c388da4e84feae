"""The reference side of the listener reports (include/sdrainer_hip.h sdr_listener_report), in numpy over what the oracle
returns: the value handed to Listener.Listen (`values`), the debounced bits (`deb`), the frame records' noise_floor, and
oracle.Decoder for the speed.  The quantisation lives here, once.  A plain helper module, not a test file."""
import numpy as np

from oracle import oracle as orc

INT32_MIN = -2 ** 31
SUM_FIELDS = ("ticks", "ticks_on", "ticks_off", "on_sum_q", "off_sum_q", "floor_sum_q")
FIELDS = ("band", "listener", "bin") + SUM_FIELDS + ("on_max_q", "wpm")


def q(x):
    """q(x) = (int32) rint(clamp(x, -1024, 1024) * 256): float32, round half to even, the product exact."""
    with np.errstate(invalid="ignore"):
        return np.rint(np.clip(x, -1024, 1024).astype(np.float32) * np.float32(256)).astype(np.int64)


def report(values, deb, noise_floor):
    """One listener's record fields over its ticks (1-d arrays of equal length): a tick is measured if neither its value nor
    its frame's noise floor is NaN."""
    v, nf = np.asarray(values, np.float32), np.asarray(noise_floor, np.float32)
    d = np.asarray(deb).astype(bool)
    assert v.shape == nf.shape == d.shape and v.ndim == 1
    measured = ~np.isnan(v) & ~np.isnan(nf)
    on, off = measured & d, measured & ~d
    qv, qn = q(np.where(measured, v, 0)), q(np.where(measured, nf, 0))
    return {"ticks": int(v.size), "ticks_on": int(on.sum()), "ticks_off": int(off.sum()),
            "on_max_q": int(qv[on].max()) if on.any() else INT32_MIN,
            "on_sum_q": int(qv[on].sum()), "off_sum_q": int(qv[off].sum()), "floor_sum_q": int(qn[on].sum())}


def add(total, rec):
    """Reports of consecutive batches add up: sums and counts add, on_max_q takes the maximum, wpm the last value."""
    if total is None:
        return dict(rec)
    out = dict(total)
    for f in SUM_FIELDS:
        out[f] = total[f] + rec[f]
    out["on_max_q"] = max(total["on_max_q"], rec["on_max_q"])
    if "wpm" in rec:
        out["wpm"] = rec["wpm"]
    return out


def wpm_at(deb_col, rate, tick_samples, ends, start=0):
    """Decoder.wpm of cw.NewDecoder(rate, tick_samples) over the debounced bits from tick `start` on, read behind tick
    e - 1 for every e of `ends` (ascending; an end at or before `start` reads the new decoder)."""
    d = orc.Decoder(rate, tick_samples)
    d.reset()
    col, pos, out = np.ascontiguousarray(deb_col, np.uint8), start, []
    for e in ends:
        if e > pos:
            d.ticks(col[pos:e])
            pos = e
        out.append(float(d.state()[3]))  # (out12[3] of sdr_read_decoder_state: Decoder.wpm)
    return out


def expected(out, band, lid, bin_, a, e, start, wpm):
    """The record of listener `lid` of `band` for the batch [a, e) from the oracle's output of that band; the listener
    listens from frame `start` on."""
    s = min(max(start, a), e)
    rec = report(out["values"][s:e, lid], out["deb"][s:e, lid], out["frames"]["noise_floor"][s:e])
    rec.update(band=band, listener=lid, bin=int(bin_), wpm=float(wpm))
    return rec


def as_dict(r):
    """A polled record (numpy void of capi.REPORT_DTYPE) as the dict `expected` builds."""
    return {f: (float(r[f]) if f == "wpm" else int(r[f])) for f in FIELDS}


def same(got, want):
    """Field by field: integers, and the bits of wpm."""
    bad = [f for f in FIELDS if (np.float64(got[f]).tobytes() != np.float64(want[f]).tobytes() if f == "wpm" else got[f] != want[f])]
    return bad
