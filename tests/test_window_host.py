"""A window on the frames (sdr_set_window) without a GPU: the symbols, synth.hann, the batch plan's rule for a windowed
bank (tests/host/test_batch_plan_window.cpp), and the oracle-only half of the demonstration the feature exists for, so
that its input is pinned where no GPU is needed (tests/test_window_gpu.py runs the bank against it).

The demonstration (192 kS/s, N = 4096, hop = 1024, one listener on bin 2600): a weak station exactly on bin 2600 keys a
call sign; a neighbour 50 dB stronger sits half-way between two bins, 11.5 bins below.  Under the rectangular window the
neighbour's leakage (falling as 1 / (pi * distance in bins)) buries the weak station: FindPeaks sees the two as one run
and the listener decodes nothing of the call sign.  Under a Hann window the two are two peaks and the call sign is read."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import oracle as orc
from sdrainer_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")
NEW_SYMBOLS = ["sdr_set_window", "sdr_group_set_window"]

DEMO = dict(rate=192_000, n=4096, hop=1024, edge=560, bin=2600, weak_amplitude=3e-4, weak_text="cq de dl1abc dl1abc dl1abc k",
            weak_repeats=2, weak_wpm=20, strong_amplitude=0.1, strong_bin=2588.5, strong_text="test w1aw w1aw test", strong_wpm=27,
            strong_edge_ms=5.0, sigma=1e-3, seed=5)


def windowed(frames, w, n):
    """Frames [F, 2N] float32 with sample i of each multiplied by w[i]: numpy's float32 product, one rounding per
    component - the definition of what the bank computes with that window."""
    w = np.asarray(w, np.float32)
    return (frames.reshape(-1, n, 2) * w[None, :, None]).astype(np.float32).reshape(-1, 2 * n)


def _carrier(bin_, n, a, e):
    """cos and sin of the carrier at spectrum bin `bin_` (a multiple of 0.5) over samples [a, e): FFT index bin_ + N / 2
    (the spectrum is fft-shifted), the phase reduced in integers."""
    k2 = int(round(2 * bin_)) + n  # twice the FFT index
    ph = np.pi * ((k2 * np.arange(a, e, dtype=np.int64)) % (2 * n)) / n
    return np.cos(ph), np.sin(ph)


def demo_stream(neighbour):
    """float32 [samples, 2]: the weak keyed station on bin 2600, the strong neighbour ("carrier": unkeyed; "soft": keyed
    with raised-cosine edges) and noise, I drawn before Q over the whole stream."""
    d = DEMO
    rate, n = d["rate"], d["n"]
    dit = int(round(1.2 / d["weak_wpm"] * rate))
    key = np.repeat(np.concatenate([np.zeros(30, np.uint8), np.tile(synth.keying_pattern(d["weak_text"], 1), d["weak_repeats"])]), dit)
    samples = (len(key) + n + 8191) // 8192 * 8192
    key = np.concatenate([key, np.zeros(samples - len(key), np.uint8)]).astype(np.float64)
    if neighbour == "carrier":
        strong = np.ones(samples)
    else:
        sdit = int(round(1.2 / d["strong_wpm"] * rate))
        pat = np.repeat(np.concatenate([synth.keying_pattern(d["strong_text"], 1), np.zeros(7, np.uint8)]), sdit)
        strong = np.tile(pat, samples // len(pat) + 1)[:samples].astype(np.float64)
        kern = np.hanning(int(round(d["strong_edge_ms"] * 1e-3 * rate)) + 2)[1:-1]
        strong = np.convolve(strong, kern / kern.sum(), mode="same")
    rng = np.random.default_rng(d["seed"])
    noise_i = d["sigma"] * rng.standard_normal(samples)
    noise_q = d["sigma"] * rng.standard_normal(samples)
    out = np.empty((samples, 2), np.float32)
    step = 1 << 21
    for a in range(0, samples, step):
        e = min(samples, a + step)
        wc, ws = _carrier(d["bin"], n, a, e)
        sc, ss = _carrier(d["strong_bin"], n, a, e)
        out[a:e, 0] = d["weak_amplitude"] * key[a:e] * wc + d["strong_amplitude"] * strong[a:e] * sc + noise_i[a:e]
        out[a:e, 1] = d["weak_amplitude"] * key[a:e] * ws + d["strong_amplitude"] * strong[a:e] * ss + noise_q[a:e]
    return out


def demo_oracle(s, w, piece=1200):
    """The oracle receiver (find_peaks on) over every frame of stream s with window w (None: rectangular), the frames
    materialised `piece` at a time, and the hop-timed decoder over the listener's debounced bits.  Returns deb bits, text,
    decoder state, and per completed cumulation its completing frame and peak list."""
    from test_overlap_gpu import decode, frames_of

    d = DEMO
    rate, n, hop = d["rate"], d["n"], d["hop"]
    r = orc.Receiver(rate, n, d["edge"])
    r.attach(d["bin"])
    frames = (s.shape[0] - n) // hop + 1
    deb, peak_frames, peaks = [], [], []
    for a in range(0, frames, piece):
        f = frames_of(s, n, hop, a, min(a + piece, frames))
        out = r.process(f if w is None else windowed(f, w, n))
        deb.append(out["deb"][:, 0])
        peak_frames += [a + int(x) for x in out["peak_frames"]]
        peaks += out["peaks"]
    deb = np.concatenate(deb)
    text, state, _ = decode(deb, rate, hop)
    return dict(deb=deb, text=text, state=state, peak_frames=peak_frames, peaks=peaks, frames=frames)


def merged_runs(peaks, lo=2588, hi=2600):
    """How many cumulations hold one peak run that contains both bins (the two stations are one peak), and the longest run."""
    merged = sum(any(p[0] <= lo and p[1] >= hi for p in pk) for pk in peaks)
    longest = max((p[1] - p[0] + 1 for pk in peaks for p in pk), default=0)
    return merged, longest


def check_demo_oracle(rect, hann):
    """The assertions on the oracle alone: they come first, so that a weak input fails as an input."""
    assert len(rect["peaks"]) == len(hann["peaks"]) >= 70
    assert "dl1abc" not in rect["text"], rect["text"]
    assert merged_runs(rect["peaks"])[0] * 2 >= len(rect["peaks"]), merged_runs(rect["peaks"])
    assert hann["text"].count("dl1abc") >= 4, hann["text"]
    assert merged_runs(hann["peaks"])[0] == 0, merged_runs(hann["peaks"])


@pytest.fixture(scope="module")
def lib():
    from sdrainer_amd.csrc import build
    return build.build()


def test_symbols_in_library_header_and_binding(lib):
    from sdrainer_amd import capi
    dyn = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dyn.splitlines() if line.strip()}
    header = open(os.path.join(ROOT, "include", "sdrainer_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in exported, f"{name} is not exported by the library"
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in the header"
        assert name in capi.SYMBOLS
    assert hasattr(capi.Bank, "set_window") and hasattr(capi.Group, "set_window")


@pytest.mark.parametrize("n", [512, 4096, 65536])
def test_hann_is_its_formula(n):
    w = synth.hann(n)
    assert w.dtype == np.float32 and w.shape == (n,)
    assert w[0] == 0.0 and w[n // 2] == 1.0
    want = np.array([np.float32(0.5 - 0.5 * np.cos(2.0 * np.pi * i / n)) for i in range(n)], np.float32)
    assert np.array_equal(w.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(w[1:], w[:0:-1])  # periodic: symmetric about n / 2, w[n - i] == w[i]
    assert abs(float(w.astype(np.float64).mean()) - 0.5) < 1e-6  # coherent gain 0.5 = -6.02 dB
    assert abs(float((w.astype(np.float64) ** 2).mean()) - 0.375) < 1e-6  # power gain 0.375 = -4.26 dB


def test_windowed_frames_are_one_float32_product():
    """The oracle side of every comparison: each component times its sample's window value, rounded once to float32."""
    rng = np.random.default_rng(3)
    n = 512
    f = rng.standard_normal((3, 2 * n)).astype(np.float32)
    w = rng.random(n, dtype=np.float32)
    got = windowed(f, w, n)
    want = (f.astype(np.float64).reshape(3, n, 2) * w.astype(np.float64)[None, :, None]).astype(np.float32).reshape(3, 2 * n)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))  # (24 x 24 bits fit a double)
    assert np.array_equal(windowed(f, np.ones(n, np.float32), n).view(np.uint32), f.view(np.uint32))


def test_batch_plan_never_puts_a_windowed_bank_on_r32(tmp_path):
    exe = str(tmp_path / "test_batch_plan_window")
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe,
                         os.path.join(HOST, "test_batch_plan_window.cpp")], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "FAILED" not in run.stdout, run.stdout + run.stderr
    assert run.stdout.split() == ["plan", "ok"]


@pytest.mark.parametrize("neighbour", ["carrier", "soft"])
def test_the_oracle_needs_the_window(neighbour):
    """Measured with the oracle over the stream's 72 cumulations - rectangular / Hann: 'dl1abc' read 0 / 6 times (unkeyed
    neighbour) and 0 / 5 times (soft-keyed, its message repeated behind a word gap for the whole stream); the two stations
    one peak run in 72 / 0 and 63 / 0 cumulations; longest run 346 / 12 and 231 / 12 bins."""
    s = demo_stream(neighbour)
    rect, hann = demo_oracle(s, None), demo_oracle(s, synth.hann(DEMO["n"]))
    print(neighbour, "rectangular:", repr(rect["text"]), merged_runs(rect["peaks"]), "hann:", repr(hann["text"]), merged_runs(hann["peaks"]),
          "cumulations", len(rect["peaks"]))
    check_demo_oracle(rect, hann)
