"""The fine converter's arithmetic restated in NumPy (include/sdrainer_hip.h "fine converter"): the oracle
of tests/test_fine_ref.py and test_fine_gpu.py.  A band is tests/ddc_ref.py's mix and tap loop applied to the input stream the
band points at; the object keeps one RAW carry of T - 1 samples per input, read or not, so a band moved to another input
finds that input's history.  The table is an argument (capi.ddc_nco_table()), as in ddc_ref.  A plain helper module, not a
test file."""
import numpy as np

import chan_ref as CR
import ddc_ref as R
from sdrainer_amd import synth

L = R.L


class FineRef:
    """process(x) takes the next n (a multiple of D) float32 samples of every input, x [inputs, n, 2], and returns float32
    [bands, n / D, 2].  steps and inputs are lists that may be changed between calls (set_nco_step, set_input): an output
    uses, for all its taps, what is current in the call that produces it.  Samples below the first sample are zero."""

    def __init__(self, n_inputs, decimation, taps, steps, cos, sin, inputs=None, first_sample=0):
        self.n_inputs, self.d, self.taps = int(n_inputs), int(decimation), np.asarray(taps, np.float32)
        self.steps = [int(s) for s in steps]
        self.inputs = list(range(len(self.steps))) if inputs is None else [int(i) for i in inputs]
        assert len(self.inputs) == len(self.steps) and all(0 <= i < self.n_inputs for i in self.inputs)
        self.cos, self.sin = np.asarray(cos, np.float32), np.asarray(sin, np.float32)
        self.total = int(first_sample)
        self.hist = np.zeros((self.n_inputs, len(self.taps) - 1, 2), np.float32)

    def set_nco_step(self, band, step):
        self.steps[band] = int(step)

    def set_input(self, band, input_):
        assert 0 <= input_ < self.n_inputs
        self.inputs[band] = int(input_)

    def process(self, x):
        x = np.asarray(x, np.float32).reshape(self.n_inputs, -1, 2)
        d, t = self.d, len(self.taps)
        n = x.shape[1]
        assert n % d == 0 and self.total % d == 0
        m = n // d
        span = np.concatenate([self.hist, x], axis=1)
        k = self.total - (t - 1) + np.arange(span.shape[1], dtype=np.int64)
        at = (t - 1) + np.arange(m) * d  # span index of sample n * D of output n
        out = np.empty((len(self.steps), m, 2), np.float32)
        for b, (step, i) in enumerate(zip(self.steps, self.inputs)):
            y = R.mix(span[i], k, step, self.cos, self.sin)
            acc = np.zeros((m, 2), np.float32)
            for j in range(t):
                acc = acc + (self.taps[j] * y[at - j])
            out[b] = acc
        self.hist = span[:, span.shape[1] - (t - 1):]
        self.total += n
        return out


def fine_ref(x, decimation, taps, steps, cos, sin, inputs=None, first_sample=0):
    """The whole streams x [inputs, n, 2] in one call."""
    x = np.asarray(x, np.float32)
    return FineRef(x.shape[0], decimation, taps, steps, cos, sin, inputs, first_sample).process(x)


def tune_ref(n_channels, decimation, target):
    """sdr_fine_tune restated with Python integers: (channel, step)."""
    q = L * decimation // n_channels
    c, r = divmod(2 * target + q, 2 * q)  # floor: a tie (r == 0) was rounded up
    if r == 0 and c % 2:
        c -= 1
    step = target - c * q
    if step == L // 2:
        c, step = c + 1, -(L // 2)
    return c % n_channels, step


# -- the end-to-end fixture: one cu8 wide stream at 1 536 000 S/s, two keyed call signs OFF the channel grid.  Stage one is a
#    channelizer of 8 channels at decimation 4 (384 kS/s per channel, centres 192 kHz apart), stage two decimates by 8 to the
#    bank's 48 kS/s.  The targets are what fine_tune turns into (channel 1, step 4800) and (channel 6, step -6400): the
#    stations lie 28 125 Hz above channel 1's centre and 37 500 Hz below channel 6's, outside a 48 kHz band round either
#    centre, so nothing decodes without the fine step.  Texts, speeds and amplitude are ddc_ref.E2E's; the wide noise is
#    twice its sigma, because the total decimation is four times ddc_ref's and unit-gain filters leave a quarter of the
#    noise power: the narrow bands then have ddc_ref.E2E's signal-to-noise ratio (with its sigma the reference decoder
#    itself splits the second call sign into letters). ----------------------------------------------------------------------
E2E = dict(R.E2E, wide_rate=1_536_000, n_channels=8, d1=4, d2=8, targets=(32768 + 4800, -2 * 32768 - 6400), channels=(1, 6),
           fine_steps=(4800, -6400), sigma=0.04)
del E2E["decimation"], E2E["steps"], E2E["taps_per_phase"]


def e2e_wide():
    """(cu8 [samples, 2], narrow samples per band): the carriers sit on bins E2E["bins"] of their bands' N-point spectra."""
    e = E2E
    total_d = e["d1"] * e["d2"]
    narrow = (e["frames"] - 1) * e["hop"] + e["n"]
    narrow += -narrow % 4
    wide = narrow * total_d
    carriers = []
    for target, bin_, text, dit in zip(e["targets"], e["bins"], e["texts"], e["dit_ticks"]):
        offset = target * e["wide_rate"] / (L * e["d1"]) + (bin_ - e["n"] // 2) * e["rate"] / e["n"]
        per_tick = e["hop"] * total_d
        key = np.repeat(np.concatenate([np.zeros(40, np.uint8), synth.keying_pattern(text, dit)]), per_tick)
        carriers.append((offset, e["amplitude"], key))
    return synth.wide_stream(wide, e["wide_rate"], carriers, noise_sigma=e["sigma"], seed=e["seed"], quantise="cu8"), narrow


def e2e_taps():
    """(stage one's prototype, stage two's low-pass)."""
    return synth.lowpass_taps(4, 8), synth.lowpass_taps(8, 8)


_E2E_CACHE = {}


def e2e_reference(cos, sin):
    """The fixture through the reference chain, computed once: (raw cu8, narrow length, stage one [2, n1, 2], narrow [2, n, 2])."""
    if "ref" not in _E2E_CACHE:
        e = E2E
        raw, narrow = e2e_wide()
        h1, h2 = e2e_taps()
        one = CR.chan_ref(R.to_f32(raw, R.CU8), e["n_channels"], e["d1"], h1, cos, sin, channels=e["channels"])
        two = fine_ref(one, e["d2"], h2, e["fine_steps"], cos, sin)
        for a in (raw, one, two):
            a.setflags(write=False)
        _E2E_CACHE["ref"] = (raw, narrow, one, two)
    return _E2E_CACHE["ref"]
