"""What the default seeds of tests/test_gpu_fuzz_features.py reach, without a GPU: the FFT kernel of every batch they make
(host/batch_plan.h, asked through tests/host/iq8_plan.cpp under each seed's own switches), their formats, deliveries, hops,
window transitions, origins, steps and adversarial kinds - and that the oracle, run alone over every seed without a silent
run, sees an edge and a peak: a seed that shows the oracle nothing proves nothing.  A later edit that shrinks the generator's
reach fails here."""
import os
import subprocess

import pytest

import fuzz_features_gen as gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = 22  # host/batch_plan.h FftKernel::COUNT
HOP_DELIVERIES = ("stream", "staged_hop")
STAGED = ("staged", "staged_hop")
DEVICE = ("device", "stream")


class Row:
    """One batch of one seed: its step, its window, where it starts and the kernel the plan picks for it."""

    def __init__(self, s, steps, i, k, pos, kernel):
        self.s, self.steps, self.step, self.k, self.pos, self.kernel = s, steps, steps[i], k, pos, kernel
        self.frames = steps[i][1]
        self.window = s.windows[k]


@pytest.fixture(scope="module")
def reach(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fft_plan") / "iq8_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "host", "iq8_plan.cpp")])
    asked = {}

    def kernel(s, frames, slots, windowed):
        args = (s.n, frames, s.n_bands, slots, int(windowed), s.fmt, s.hop if s.hop < s.n else 0)
        key = args + tuple(sorted(s.env.items()))
        if key not in asked:
            env = {k: v for k, v in os.environ.items() if not k.startswith("SDR_")}
            env.update({k: str(v) for k, v in s.env.items()})
            w = subprocess.check_output([exe] + [str(a) for a in args], text=True, env=env).split()
            got = dict(zip(w[0::2], w[1::2]))
            asked[key] = (int(got["id"]), got["kernel"])
        return asked[key]

    seeds = [gen.Seed(i) for i in range(gen.DEFAULT_SEEDS)]
    rows = []
    for s in seeds:
        steps, init = s.steps([[100 + 8 * i for i in range(s.tones)]] * s.n_bands)  # (the bins do not change the plan)
        slots = [len(x) for x in init]  # the slot pool is a high-water mark
        pos = k = 0
        for i, st in enumerate(steps):
            if st[0] == "attach":
                slots[st[1]] += 1
            elif st[0] in ("batch", "defer"):
                rows.append(Row(s, steps, i, k, pos, kernel(s, st[1], max(slots), s.windows[k] is not None)))
                for band, _, _ in st[2] if st[0] == "defer" else []:
                    slots[band] += 1
                pos, k = pos + st[1], k + 1
    return seeds, rows


def _phases(windows, unit=1):
    """The window of every batch reduced to the sequence of changes: tables by identity, None as it is."""
    out = []
    for w in windows[::unit]:
        if not out or out[-1] is not w:
            out.append(w)
    return out


def _transition(s):
    """The transition a seed's windows make, read from the tables themselves."""
    ph = _phases(s.windows)
    if len(ph) == 1:
        return "none" if ph[0] is None else "A"
    if len(ph) == 2:
        return "0A" if ph[0] is None else ("A0" if ph[1] is None else "AB")
    assert len(ph) == 3 and ph[1] is None and ph[0] is ph[2]
    return "A0A"


def test_every_fft_kernel_is_reached(reach):
    _, rows = reach
    got = {}
    for r in rows:
        got.setdefault(r.kernel[0], (r.kernel[1], r.s.seed))
    assert sorted(got) == list(range(KERNELS)), f"FftKernel ids not reached: {sorted(set(range(KERNELS)) - set(got))}"
    # k_fft_r32_hop* once by the plan's own rule, not by the switch
    assert any(r.kernel[1].startswith("k_fft_r32_hop") and not r.s.env for r in rows), "k_fft_r32_hop* by the plan's own rule"
    for name in ("k_fft_r32", "k_fft_r32_sc16", "k_fft_r32_iq8", "k_fft_r32_hop", "k_fft_r32_hop_sc16", "k_fft_r32_hop_iq8"):
        assert any(r.kernel[1] == name for r in rows), name


def test_every_format_and_delivery_is_reached(reach):
    seeds, _ = reach
    pairs = {(s.fmt, s.delivery) for s in seeds}
    want = {(f, d) for f in gen.FORMATS for d in gen.DELIVERIES[:5]} | {("sc16", "kiwi")}
    assert pairs >= want, sorted(want - pairs)
    assert {s.n for s in seeds} == set(gen.SIZES)
    assert any(s.pad for s in seeds if s.delivery == "stream") and any(not s.pad for s in seeds if s.delivery == "stream")
    for s in seeds:
        assert (s.hop < s.n) == (s.delivery in HOP_DELIVERIES) and gen.hop_valid(s.hop, s.n)
        assert s.trace or s.hop == s.n, "a seed with a hop runs with trace"
        assert s.n_bands <= (3 if s.n <= 16384 else 2)
        assert (s.total - 1) * s.hop + s.n <= 1 << 24 and (not s.trace or s.total <= 640)
    assert any(s.trace for s in seeds if s.hop == s.n) and any(not s.trace for s in seeds)


def test_staged_hops_and_hop_ratios_are_reached(reach):
    seeds, _ = reach
    staged = [s for s in seeds if s.delivery == "staged_hop"]
    assert {gen.family(s.n) for s in staged} == {"psd", "16384", "2p"}
    assert {s.fmt for s in staged} == set(gen.FORMATS)
    ratios = {(s.n // s.hop, s.n) for s in seeds if s.hop < s.n}
    assert {r for r, _ in ratios} == {2, 4, 8, 16}
    assert (16, 512) in ratios and (16, 65536) in ratios
    assert all(s.tones == 1 for s in seeds if s.hop == 32) and all(s.tones == 2 for s in seeds if s.hop >= 64)


def test_every_window_transition_is_reached(reach):
    seeds, rows = reach
    for s in seeds:
        assert _transition(s) == s.transition, s.ident()
        if s.graph:
            assert all(len(_phases(s.windows[i:i + gen.GRAPH_BATCHES])) == 1 for i in range(0, len(s.windows), gen.GRAPH_BATCHES)), \
                "a window changes inside a replay"
    for tr in gen.TRANSITIONS[1:]:
        assert any(s.transition == tr and s.delivery in DEVICE for s in seeds), f"{tr} on a device path"
        assert any(s.transition == tr and s.delivery in STAGED for s in seeds), f"{tr} on a staged path"
    for tr in ("AB", "A0"):
        assert any(s.transition == tr and s.graph for s in seeds), f"{tr} between graph replays"
    windowed = {(r.s.fmt, gen.family(r.s.n)) for r in rows if r.window is not None}
    assert windowed == {(f, fam) for f in gen.FORMATS for fam in ("psd", "16384", "2p")}
    hard = {gen.family(r.s.n) for r in rows if r.window is not None and r.s.hard}
    assert hard == {"psd", "16384", "2p"}
    for s in seeds:
        for w in s.tables.values() if s.hard else []:
            zeros, negative = float((w == 0).mean()), float((w < 0).mean())
            assert 0.05 < zeros < 0.15 and 0.05 < negative < 0.15 and bool(abs(w).max() < 1) and w.dtype.name == "float32"


def _has_attach_at(steps):
    return any(st[0] == "defer" and st[2] for st in steps)


def test_origins_and_steps_are_reached(reach):
    seeds, rows = reach
    by_seed = {}
    for r in rows:
        by_seed.setdefault(r.s.seed, []).append(r)
    crossed = set()
    for s in seeds:
        assert s.first_frame % 100 == 0
        c = s.crossing()
        if c is not None and s.hop < s.n and _has_attach_at(by_seed[s.seed][0].steps):
            assert 0 < c < s.total
            crossed.add((s.first_frame + c) // gen.O31)
    assert crossed >= {1, 2}, "a first frame across 2^31 and one across 2^32, with a hop and sdr_attach_at"
    assert any(s.first_frame and s.crossing() is None for s in seeds)
    hard = [r for r in rows if r.s.fmt != "f32" and r.s.hop < r.s.n]
    assert any(r.frames == 1 for r in hard), "a one-frame batch"
    assert any(r.pos % 100 + r.frames > 100 for r in hard), "a batch across a cumulation boundary"
    assert any(r.step[0] == "defer" and any(r.pos <= at < r.pos + r.frames for _, _, at in r.step[2]) for r in hard), "sdr_attach_at inside a deferred batch"
    assert any(st[0] == "stop" for r in hard for st in r.steps), "sdr_listener_stop"
    assert any(st[0] == "attach" for r in hard for st in r.steps), "sdr_attach between batches"
    loose = [r for r in rows if not r.s.timed and not r.s.graph]
    assert any(st[0] == "detach" for r in loose for st in r.steps)
    assert {st[1] for r in loose for st in r.steps if st[0] == "set"} == {"peak_threshold", "signal_debounce", "edge_width", "find_peaks"}
    assert all(st[0] not in ("detach", "set") for r in rows if r.s.timed for st in r.steps), "no detach with a hop or with trace"
    # the switches: set on N <= 16384 only, SDR_FFT_FPW where the multi-frame workgroup then runs
    for s in seeds:
        if "SDR_FFT_R32" in s.env:
            assert s.n == 16384
        if "SDR_FFT_FPW" in s.env:
            assert s.fmt == "f32" and s.n in (512, 1024) and any(
                r.frames >= 515 and gen.frames_per_wg(s.env["SDR_FFT_FPW"], r.frames, s.n_bands) == s.env["SDR_FFT_FPW"] for r in by_seed[s.seed])


def test_every_adversarial_kind_is_reached(reach):
    seeds, _ = reach
    kinds = {(s.kind, s.fmt) for s in seeds if s.kind != "none"}
    assert kinds >= {("silent", "f32"), ("silent", "sc16"), ("silent", "cs8"), ("full_scale", "sc16"), ("full_scale", "cs8"),
                     ("full_scale", "cu8")}, kinds
    assert all((s.kind != "none") == (s.seed % 3 == 2) for s in seeds)


@pytest.mark.parametrize("seed", [i for i in range(gen.DEFAULT_SEEDS) if gen.Seed(i).kind != "silent"])
def test_the_oracle_sees_edges_and_peaks(seed):
    case, _ = gen.case_of(gen.Seed(seed))
    edges, peaks = case.oracle_counts()
    assert edges >= 1 and peaks >= 1, f"{edges} edges, {peaks} peaks: the seed shows the oracle nothing"
