"""Hostile keying for the GPU Morse decoder (tests/test_keying_gpu.py, the hostile row of tests/test_reports_gpu.py) and
what the CPU reach test (tests/test_keying_reach.py) reads of it: key-state streams, bands of carriers keyed by them, and
the table of cases - seeds, kinds per listener, steps - that both sides share, so that the reach test asserts on the very
inputs the GPU tests run.  A plain helper module, not a test file: numpy and the CPU oracle only, nothing of the GPU.

`stream` makes one listener's key states.  The kinds "clean", "jitter", "long" and "noise" mirror kinds 0 - 3 of make_stream
in tests/emu/emu_stages.cpp (same branches and shares, numpy's generator in place of its xorshift): the two families belong
together - a kind added to one belongs in the other.  The Morse-like kinds change their speed inside the stream."""
import functools

import numpy as np

from oracle import oracle as orc
from parity_tools import decode
from sdrainer_amd import synth

KINDS = ("clean", "jitter", "long", "noise", "fast", "dahs", "sparse", "silent")
LEAD = 80  # silent frames in front of every band: both 60-frame rolling means fill before the first mark
N, RATE = 512, 48_000
TEXT_CAP = 2048  # runes a listener's text buffer holds between reads


def stream(ticks, kind, rng, dits=None, symbols=None):
    """uint8 [ticks] key states of one carrier.
      clean   Morse-like: characters of 1 - 6 symbols, word gaps, long silences (the abort check), over-long marks,
              glitches of one tick, a new speed now and then (dit = 2 - 11 ticks)           (emu_stages kind 0)
      jitter  the same with every run a tick shorter or longer at random                     (kind 1)
      long    jitter with up to 10 symbols per character: the ninth-symbol rule              (kind 2)
      noise   short runs of either state, now and then one of up to 300 ticks                (kind 3)
      fast    clean at a dit of 2 - 3 ticks, three symbols of four a dit, four draws of five a character and the long
              silences shorter: some 250 edges per 1024 ticks, where the other kinds make 100
      dahs    clean at a dit of 2 - 5 ticks where a character is 9 - 16 dah-length marks with dit gaps
      sparse  marks and silences of hundreds of ticks: 0 - 2 edges per 1024 ticks
      silent  no mark at all
    dits: (lowest, highest) dit of the Morse-like kinds, in place of the kind's own; symbols: the most symbols of a
    character, likewise."""
    assert kind in KINDS, kind
    out = np.zeros(ticks, np.uint8)
    if kind == "silent":
        return out
    pos = 0

    def r(k):
        return int(rng.integers(0, k))

    def push(v, length):
        nonlocal pos
        if v:
            out[pos:pos + length] = 1
        pos += length

    if kind == "sparse":
        while pos < ticks:
            push(0, 300 + r(900))
            push(1, 200 + r(600))
        return out
    if kind == "noise":
        while pos < ticks:
            push(r(2), 1 + r(6) if r(50) else 1 + r(300))
        return out
    lo, hi = dits or {"fast": (2, 3), "dahs": (2, 5)}.get(kind, (2, 11))

    def new_dit():
        return lo + r(hi - lo + 1)

    def jit(length):
        return max(1, length + (r(3) - 1 if kind in ("jitter", "long") else 0))

    fast = kind == "fast"
    shares = (80, 88, 91, 94, 97) if fast else (55, 70, 78, 84, 92)  # characters, word gaps, silences, over-long marks, glitches
    dit = new_dit()
    while pos < ticks:
        what = r(100)
        if what < shares[0]:
            if kind == "dahs" and r(2):
                marks = [3 * dit] * (9 + r(8))
            else:
                marks = [dit if r(4 if fast else 2) else 3 * dit for _ in range(1 + r(symbols or (10 if kind == "long" else 6)))]
            for m in marks:
                push(1, jit(m))
                push(0, jit(dit))
            push(0, jit(2 * dit))
        elif what < shares[1]:
            push(0, jit(7 * dit))
        elif what < shares[2]:
            push(0, 12 * dit + r((20 if fast else 40) * dit))
        elif what < shares[3]:
            push(1, 8 * dit + r(20 * dit))
            push(0, jit(dit))
        elif what < shares[4]:
            for _ in range(1 + r(3)):
                push(r(2), 1)  # glitches
        else:
            dit = new_dit()
    return out


def key_matrix(frames, kinds, seed, dits=None, symbols=None, lead=LEAD):
    """uint8 [frames, len(kinds)]: `lead` silent frames, then every column its kind's stream (a generator per column, so that
    a column does not depend on its neighbours)."""
    keys = np.zeros((frames, len(kinds)), np.uint8)
    for i, kind in enumerate(kinds):
        keys[lead:, i] = stream(frames - lead, kind, np.random.default_rng([seed, i]), dits, symbols)
    return keys


def keyed_band(n, rate, keys, seed, amplitude=synth.TONE_AMPLITUDE, hop=None, lead=LEAD, sigma=synth.NOISE_SIGMA):
    """(float32 frames [F, 2N], None, the carriers' bins): what Case(bands=...) takes.  One carrier per column of keys [F, L]
    on synth.tone_bins (the last noise window kept free), hard-keyed per frame, built as synth.make_band builds its bands:
    the inverse FFT of a sparse spectrum plus `sigma` (synth.NOISE_SIGMA) of noise.  The sample rate takes no part: the keying is given
    in frames.
    hop (below n, a divisor of it): keys has a row per hop; the rows are built at block size `hop` and flattened into one
    continuous stream float32 [F * hop, 2], as parity_tools.make_stream does - every carrier makes whole cycles per hop, and
    bin i of the short transform is bin i * n / hop of the long one.  Frame f of the stream is rows f .. f + n / hop - 1.
    lead: the frames in front that must be silent (a caller that wants keying while the rolling means still fill - the
    oracle and the bank agree there too, only the keying is not what was sent - passes 0 here and to key_matrix)."""
    del rate
    keys = np.asarray(keys, np.uint8)
    assert not keys[:lead].any(), f"the first {lead} frames are silent"
    size = hop or n
    assert n % size == 0
    bins = synth.tone_bins(size, keys.shape[1], free_last_window=True)
    rng = np.random.default_rng(seed)
    fft_bins = (bins + size // 2) % size
    iq = np.empty((keys.shape[0], 2 * size), np.float32)
    for a in range(0, keys.shape[0], 4096):
        k = keys[a:a + 4096]
        spec = np.zeros((k.shape[0], size), np.complex128)
        spec[:, fft_bins] = amplitude * size * k.astype(np.float64)
        x = np.fft.ifft(spec, axis=1)
        x += sigma * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))
        iq[a:a + 4096, 0::2] = x.real
        iq[a:a + 4096, 1::2] = x.imag
    if hop:
        iq = iq.reshape(-1, 2)
    return iq, None, [int(b) * (n // size) for b in bins]


def oracle_bits(n, rate, frames, bins, debounce=1, hop=None):
    """The oracle receiver's debounced bits uint8 [F, len(bins)] over frames [F, 2N] (with a hop: a stream [samples, 2])."""
    from parity_tools import frames_of

    r = orc.Receiver(rate, n, synth.default_edge_width(n), 15.0, debounce)
    for b in bins:
        r.attach(int(b))
    r.set_find_peaks(False)
    return r.process(frames_of(frames, n, hop) if hop else frames)["deb"]


def edge_frames(deb_col):
    """The frames at which a column of debounced bits changes (the state before frame 0 is key-up)."""
    return np.flatnonzero(np.diff(np.concatenate([[0], deb_col.astype(np.int8)])) != 0)


def anatomy(deb_col, rate, tick_samples, start=0):
    """oracle.Decoder(rate, tick_samples) ticked over one listener's debounced bits from frame `start` on, read behind
    every tick.  Returns a dict:
      edges    one (frame, state, run, invalid, symbol, da) per edge - run: the ticks of the run the edge ends; for a falling
               edge whether the mark is over-long (cw/decode.go:287: at least twice the mark threshold's high, behind its Put),
               whether it appends a symbol, and whether that is a da (at least the mark threshold)
      runes    one (frame, rune) per rune written, in order
      wpm      Decoder.wpm behind the last tick"""
    d = orc.Decoder(rate, tick_samples)
    d.reset()
    L, col = orc.lib(), np.ascontiguousarray(deb_col, np.uint8)
    edges, runes, have, last, run_start = [], [], 0, 0, start
    for f in range(start, len(col)):
        L.orc_decoder_tick(d._h, int(col[f]))
        now = L.orc_decoder_out_len(d._h)
        if now > have:
            out = L.orc_decoder_out(d._h)
            runes += [(f, chr(out[i])) for i in range(have, now)]
            have = now
        if col[f] != last:
            run = f - run_start
            invalid = symbol = da = False
            if not col[f] and run >= 2:  # (kMinDitTime)
                st = d.state()
                invalid = run >= 2 * st[5]
                symbol = not invalid
                da = symbol and run >= st[7]
            edges.append((f, int(col[f]), run, invalid, symbol, da))
            last, run_start = col[f], f
    return {"edges": edges, "runes": runes, "wpm": float(d.wpm)}


# -- (a) base --------------------------------------------------------------------------------------------------------------
# Two bands of 19 carriers on a bank of max_listeners = 19: 38 slots - k_listen_decode's second workgroup of 16 holds the
# last three of band 0 and the first thirteen of band 1, its third six listeners.  (A bank of 19 listeners per band has
# no twentieth slot: the carrier without a listener is band 0's nineteenth, not an additional one.)  The kind of a slot follows from its place
# in its workgroup, so every workgroup has fast, dahs, sparse and silent listeners side by side.  Band 0's last carrier
# (slot 18, a "long" one) has no listener until the ("attach", ...) step: until then its half-wave partner, slot 19, works
# alone; afterwards slot 18 starts inside a stream of characters.
A_SEED, A_FRAMES, A_LISTENERS = 7100, 4500, 19
A_PLACE = ("fast", "dahs", "long", "sparse", "silent", "clean", "jitter", "noise", "fast", "dahs", "sparse", "long", "clean",
           "jitter", "silent", "fast")
A_CUT_LISTENER = (0, 0)  # (band, listener): the fast one whose edges place two of the cuts
A_LATE = 18              # band 0's carrier that gets its listener late


def a_kinds(band):
    return [A_PLACE[(band * A_LISTENERS + i) % 16] for i in range(A_LISTENERS)]


@functools.lru_cache(maxsize=None)
def a_bands():
    return [keyed_band(N, RATE, key_matrix(A_FRAMES, a_kinds(b), A_SEED + b), A_SEED + 10 + b) for b in range(2)]


@functools.lru_cache(maxsize=None)
def a_steps():
    """1024 frames; cuts of 1, 63, 64 and 65; a batch that ends where the cut listener's 65th edge of it would be (64 edges,
    the next batch begins with an edge); one that ends behind its 33rd edge; the late listener; 1024 twice; the rest."""
    band, lid = A_CUT_LISTENER
    f32, _, bins = a_bands()[band]
    ed = edge_frames(oracle_bits(N, RATE, f32, bins[:lid + 1])[:, lid])
    steps, pos = [], 0
    for x in (1024, 1, 63, 64, 65):
        steps.append(("batch", x))
        pos += x
    after = ed[ed >= pos]
    e64, e33 = int(after[64]), int(after[64 + 32]) + 1
    steps += [("batch", e64 - pos), ("batch", e33 - e64), ("attach", 0, bins[A_LATE]), ("batch", 1024), ("batch", 1024)]
    steps.append(("batch", A_FRAMES - e33 - 2048))
    assert steps[-1][1] > 0
    return tuple(steps)


def case_a(**kw):
    from parity_case import Case

    bands = a_bands()
    init = [bands[0][2][:A_LATE], bands[1][2]]
    return Case(N, 2, None, 0, list(a_steps()), A_SEED, rate=RATE, max_listeners=A_LISTENERS, bands=list(bands), init_bins=init,
                path="device", trace=True, **kw)


def band0_case(**kw):
    """(a)'s band 0 alone with its batches: the hostile row of tests/test_reports_gpu.py."""
    from parity_case import Case

    band = a_bands()[0]
    return Case(N, 1, None, 0, list(a_steps()), A_SEED, rate=RATE, max_listeners=A_LISTENERS, bands=[band], init_bins=[band[2][:A_LATE]],
                path="device", **kw)


# -- (b) debounce ----------------------------------------------------------------------------------------------------------
# (debounce, batches): 12 listeners, noise and jitter by turns.  The row of 4200 frames in one batch takes stage 0 into its
# second 64-word chunk; B_LONG names it.
B_SEED = 7200
B_ROWS = ((2, (1000, 1000)), (3, (700, 1300)), (5, (1000, 1000)), (9, (1300, 700)), (70, (1000, 1000)), (3, (4200,)))
B_LONG = 5
B_KINDS = ("noise", "jitter") * 6


@functools.lru_cache(maxsize=None)
def b_band(row):
    frames = sum(B_ROWS[row][1])
    return keyed_band(N, RATE, key_matrix(frames, B_KINDS, B_SEED + row), B_SEED + 50 + row)


def case_b(row):
    from parity_case import Case

    debounce, steps = B_ROWS[row]
    band = b_band(row)
    return Case(N, 1, None, 0, [("batch", x) for x in steps], B_SEED, rate=RATE, max_listeners=len(B_KINDS), bands=[band],
                init_bins=[band[2]], debounce=debounce, path="device", trace=True)


# -- (c) deferred ----------------------------------------------------------------------------------------------------------
# Eight carriers; the listeners of carriers 0 (fast), 1 (long) and 2 (fast) are bound by sdr_attach_at inside the deferred
# second batch, at its frames 64, 130 and its last one.
C_SEED, C_STEPS = 7306, (300, 1024, 300)
C_KINDS = ("fast", "long", "fast", "clean", "dahs", "jitter", "sparse", "noise")
C_LATE = ((0, 64), (1, 130), (2, 1023))  # (carrier, frame of the deferred batch)


@functools.lru_cache(maxsize=None)
def c_band():
    return keyed_band(N, RATE, key_matrix(sum(C_STEPS), C_KINDS, C_SEED), C_SEED + 50)


def case_c():
    from parity_case import Case

    band = c_band()
    bins = band[2]
    late = [(0, bins[i], C_STEPS[0] + at) for i, at in C_LATE]
    steps = [("batch", C_STEPS[0]), ("defer", C_STEPS[1], late), ("batch", C_STEPS[2])]
    return Case(N, 1, None, 0, steps, C_SEED, rate=RATE, max_listeners=len(C_KINDS), bands=[band], init_bins=[bins[len(C_LATE):]],
                path="device", trace=True)


# -- (d) other schedules ---------------------------------------------------------------------------------------------------
D_SEED = 7400
D_KINDS = ("fast", "dahs", "long", "sparse", "silent", "clean", "jitter", "noise", "fast", "dahs", "long", "jitter")
D_GRAPH_STEPS = (256,) * 12  # two replays of six batches
D_HOP_N, D_HOP, D_HOP_RATE, D_HOP_STEPS = 2048, 512, 192_000, (1024, 1, 65, 1010)
D_HOP_KINDS = ("clean", "dahs", "long", "sparse", "jitter", "clean", "long", "jitter")
D_HOP_DITS = (5, 10)  # a frame spans four hops: a carrier is up while any of them is, so gaps lose three ticks


def case_d_graph():
    from parity_case import Case

    band = keyed_band(N, RATE, key_matrix(sum(D_GRAPH_STEPS), D_KINDS, D_SEED), D_SEED + 50)
    return Case(N, 1, None, 0, [("batch", x) for x in D_GRAPH_STEPS], D_SEED, rate=RATE, max_listeners=len(D_KINDS), bands=[band],
                init_bins=[band[2]], path="graph", trace=True)


def case_d_hop():
    from parity_case import Case

    n, hop = D_HOP_N, D_HOP
    rows = sum(D_HOP_STEPS) - 1 + n // hop
    band = keyed_band(n, D_HOP_RATE, key_matrix(rows, D_HOP_KINDS, D_SEED + 1, D_HOP_DITS), D_SEED + 51, hop=hop)
    return Case(n, 1, None, 0, [("batch", x) for x in D_HOP_STEPS], D_SEED, rate=D_HOP_RATE, max_listeners=len(D_HOP_KINDS), bands=[band],
                init_bins=[band[2]], path="device", hop=hop, trace=True)


# -- (e) stop inside a character -------------------------------------------------------------------------------------------
# Listener 0 is keyed by hand at a dit of 3 frames: words that settle both thresholds, then a dit, a dah - E_CUTS[0] lies two
# frames behind the dah: "a" is pending - a gap, a mark of 60 frames - E_CUTS[1] lies two frames behind it: the pending
# character is invalid, its last mark is the over-long one - and more words.  The other listeners take generated kinds.
E_SEED, E_FRAMES, E_DIT = 7500, 1400, 3
E_KINDS = ("clean", "jitter", "long", "fast", "dahs")


@functools.lru_cache(maxsize=None)
def e_input():
    """(band, (cut of the ordinary pending character, cut of the invalid one))."""
    d = E_DIT
    head = synth.keying_pattern("cq de dl1abc k", d)
    hand = np.concatenate([head, np.ones(d), np.zeros(d), np.ones(3 * d)]).astype(np.uint8)
    cut_a = LEAD + len(hand) + 2
    hand = np.concatenate([hand, np.zeros(d), np.ones(60)]).astype(np.uint8)
    cut_b = LEAD + len(hand) + 2
    hand = np.concatenate([hand, np.zeros(7 * d), head]).astype(np.uint8)
    keys = key_matrix(E_FRAMES, ("silent",) + E_KINDS, E_SEED)
    keys[LEAD:LEAD + len(hand), 0] = hand[:E_FRAMES - LEAD]
    return keyed_band(N, RATE, keys, E_SEED + 50), (cut_a, cut_b)


# -- (f) text capacity -----------------------------------------------------------------------------------------------------
# Three fast listeners and a clean one in one workgroup, batches of 1024 frames, nothing read before the end.
F_SEED, F_BATCH, F_OVER = 7600, 1024, 100
F_KINDS = ("fast", "fast", "fast", "clean")
F_MAX_BATCHES = 64
F_SYMBOLS = 2  # characters of one or two symbols: the buffers fill in some thirty batches


@functools.lru_cache(maxsize=None)
def f_input():
    """(band, batches, per listener (text, the frame that wrote each rune)): as many batches as it takes every fast
    listener's text to pass TEXT_CAP by F_OVER runes - by the oracle; a decoder over the key states themselves says how
    many to build first."""
    keys = key_matrix(F_MAX_BATCHES * F_BATCH, F_KINDS, F_SEED, symbols=F_SYMBOLS)

    def batches_for(bits):
        at = [decode(bits[:, i], RATE, N)[2] for i, kind in enumerate(F_KINDS) if kind == "fast"]
        assert all(len(x) >= TEXT_CAP + F_OVER for x in at), "the fast listeners write too little"
        return max(int(x[TEXT_CAP + F_OVER - 1]) for x in at) // F_BATCH + 1

    built = min(F_MAX_BATCHES, batches_for(keys) + 2)
    band = keyed_band(N, RATE, keys[:built * F_BATCH], F_SEED + 50)
    deb = oracle_bits(N, RATE, band[0], band[2])
    batches = batches_for(deb)
    end = batches * F_BATCH
    decs = [decode(deb[:end, i], RATE, N) for i in range(len(F_KINDS))]
    return (np.ascontiguousarray(band[0][:end]), None, band[2]), batches, [(text, at) for text, _, at in decs]
