"""Banks that start at a frame just below 2^31, 2^32 and 5 * 2^32 (sdr_set_first_frame): the table of cases that
tests/test_frame_origin_gpu.py runs on the GPU and tests/test_frame_origin_reach.py holds to the CPU oracle alone - origins,
inputs, steps - so that the reach test asserts on the very inputs the GPU tests run.  A plain helper module, not a test
file: numpy and the CPU oracle only, nothing of the GPU.

The crossing of an origin is the stream frame whose bank frame index is the next multiple of 2^31: 48, 96 and 80 frames in.
A rune has to be written in front of it, and the reference's two 60-frame rolling means divide by 60 from the first frame on:
for some 35 frames every bin lies above its threshold, and a decoder's first character ends behind frame 50.  So every band
here opens with BURST frames of a wide-band burst 60 dB up (the samples times 1000): the means are filled by frame BURST,
the noise falls below the threshold there, and carrier 0, keyed by hand with marks of six frames and more (a debounce of 5
passes them), writes its first characters at frames 36 and 52 (40 and 56 at debounce 5).  The other carriers take
keying_gen's kinds from the burst on."""
import functools

import numpy as np

import keying_gen as gen
from parity_case import Case
from parity_tools import sc16_to_float32
from sdrainer_amd import synth

ORIGINS = (2147483600, 4294967200, 21474836400)  # 2^31 - 48, 2^32 - 96, 5 * 2^32 - 80: multiples of 100
O31, O32, O5 = ORIGINS
N, RATE = 512, 48_000
WIDE_N, WIDE_RATE = 2048, 192_000  # the same tick, 10.67 ms
FRAMES = 600
BURST, BURST_GAIN = 24, 1000.0
KINDS = ("silent", "fast", "dahs", "clean", "fast", "jitter")  # (carrier 0's column is replaced by the hand keying)
HAND = ((36, 42), (52, 58), (70, 90))  # carrier 0's first marks; from frame 100 on words at a dit of 6 frames
HAND_TEXT = "cq de dl1abc dl1abc k  "


def crossing(origin):
    """The stream frame whose bank frame index is the first multiple of 2^31 behind `origin`."""
    return (-origin) % (1 << 31)


def keys_of(frames, seed, kinds=KINDS, dit=6, hand=HAND, burst=BURST, words_from=100):
    keys = gen.key_matrix(frames, kinds, seed, lead=0)
    keys[:burst] = 0
    keys[:, 0] = 0
    for a, e in hand:
        keys[a:e, 0] = 1
    words = synth.keying_pattern(HAND_TEXT, dit)
    tail = np.tile(words, (frames - words_from) // len(words) + 1)[:frames - words_from]
    keys[words_from:, 0] = tail
    return keys


@functools.lru_cache(maxsize=None)
def band(n=N, rate=RATE, seed=8100, sc16=False):
    """(float32 frames [FRAMES, 2N], their int16 values or None, the carriers' bins): what Case(bands=...) takes."""
    f32, _, bins = gen.keyed_band(n, rate, keys_of(FRAMES, seed), seed + 50, lead=0)
    f32 = f32.copy()
    f32[:BURST] *= np.float32(BURST_GAIN)
    q = None
    if sc16:
        q = np.rint(f32.astype(np.float64) * (30000.0 / float(np.abs(f32).max()))).astype(np.int16)
        f32 = sc16_to_float32(q)
    return f32, q, bins


def noise_bin(n, bins):
    """A bin far from every carrier: the idle listener's."""
    return next(b for b in range(n // 2 + 5, n) if all(abs(b - c) > 8 for c in bins))


def cuts(origin, where):
    """The two cuts of the eager stream: "on" - the crossing on a batch boundary, a one-frame batch behind it; "in" - the
    crossing inside the second batch, 11, 59 or 43 frames in: at no 64-frame word end."""
    c = crossing(origin)
    head = (c, 1, 151) if where == "on" else (37, 200)
    assert where == "on" or (37 < c < 237 and (c - 37) % 64 != 0)
    return head + (FRAMES - sum(head),)


def eager(origin, where, debounce):
    b = band()
    return Case(N, 1, None, 0, [("batch", x) for x in cuts(origin, where)], 8100, rate=RATE, bands=[b],
                init_bins=[b[2] + [noise_bin(N, b[2])]], debounce=debounce, trace=True, first_frame=origin)


def attach_detach(origin):
    """Listeners 0 - 3 on carriers 0, 2, 3 and the noise bin.  At the batch boundary 16 frames before the crossing carrier 1
    gets a listener (a new slot) and listener 2 is detached; at the boundary on the crossing carrier 4 gets one, in listener
    2's slot: a brand-new decoder whose start frame is the multiple of 2^31 itself; one frame on, carrier 5 (a new slot)."""
    b = band()
    bins, c = b[2], crossing(origin)
    steps = [("batch", c - 16), ("attach", 0, bins[1]), ("detach", 0, 2), ("batch", 16), ("attach", 0, bins[4]), ("batch", 1),
             ("attach", 0, bins[5]), ("batch", 200), ("batch", FRAMES - c - 201)]
    return Case(N, 1, None, 0, steps, 8100, rate=RATE, bands=[b], init_bins=[[bins[0], bins[2], bins[3], noise_bin(N, bins)]],
                first_frame=origin)


@functools.lru_cache(maxsize=None)
def stop_cut():
    """A frame behind every crossing, two frames behind a mark of carrier 0, where Decoder.stop() writes a character."""
    from oracle import oracle as orc

    b = band()
    deb = gen.oracle_bits(N, RATE, b[0], b[2][:1])[:, 0]
    for f in gen.edge_frames(deb):
        if f > 150 and not deb[f] and not deb[f:f + 3].any():
            d = orc.Decoder(RATE, N)
            d.reset()
            d.ticks(deb[:f + 2])
            before = d.text()
            d.stop()
            if len(d.text()) > len(before) and d.text()[-1] not in " \xa6":
                return int(f) + 2
    raise AssertionError("no cut with a pending character")


def stop(origin):
    """sdr_listener_stop of listener 0 between two batches behind the crossing: the rune it writes is stamped with the last
    frame processed, and arrives with the next batch."""
    b = band()
    cut = stop_cut()
    steps = [("batch", 37), ("batch", cut - 37), ("stop", 0, 0), ("batch", FRAMES - cut)]
    return Case(N, 1, None, 0, steps, 8100, rate=RATE, bands=[b], init_bins=[b[2]], trace=True, first_frame=origin)


DEFER = (30, 230)  # the deferred batch: it straddles every crossing


def late_frames(origin):
    """start frames inside the waiting batch: before the crossing, exactly at it, behind it, and the next frame."""
    c = crossing(origin)
    return (c - 5, c, c + 7, DEFER[1])


def deferred(origin, wide=False):
    """Carriers 1 - 4 are bound by sdr_attach_at inside the deferred batch, which straddles the crossing; carrier 0, carrier 5
    and the noise bin listen from the first frame.  wide: two bands of N = 2048 (the listeners of both bound late)."""
    n, rate, n_bands = (WIDE_N, WIDE_RATE, 2) if wide else (N, RATE, 1)
    bands = [band(n, rate, 8100 + 7 * k) for k in range(n_bands)]
    late = [(k, bands[k][2][1 + i], at) for k in range(n_bands) for i, at in enumerate(late_frames(origin))]
    steps = [("batch", DEFER[0]), ("defer", DEFER[1] - DEFER[0], late), ("batch", FRAMES - DEFER[1])]
    init = [[b[2][0], b[2][5], noise_bin(n, b[2])] for b in bands]
    return Case(n, n_bands, None, 0, steps, 8100, rate=rate, bands=bands, init_bins=init, trace=True, first_frame=origin)


GRAPH_PER = 40  # one replay of six batches: cursors at 0, 40, 80 in front of the crossing at 96, 120, 160, 200 behind it


def graph(origin, sc16):
    b = band(sc16=sc16)
    b = (np.ascontiguousarray(b[0][:6 * GRAPH_PER]), None if b[1] is None else np.ascontiguousarray(b[1][:6 * GRAPH_PER]), b[2])
    return Case(N, 1, None, 0, [("batch", GRAPH_PER)] * 6, 8100, rate=RATE, bands=[b], init_bins=[b[2] + [noise_bin(N, b[2])]],
                path="graph_sc16" if sc16 else "graph", trace=True, first_frame=origin)


HOP = 128
HOP_CALLS = (300, 130)
HOP_BURST = 24
HOP_HAND = ((36, 64), (100, 128), (160, 240))  # marks of 28 hops and more: a dit is 23 ticks of 2.67 ms at 20 WPM


@functools.lru_cache(maxsize=None)
def hop_band():
    """A continuous stream float32 [samples, 2] built at block size HOP (keying_gen.keyed_band with a hop), a row per hop,
    the first HOP_BURST rows 60 dB up."""
    rows = sum(HOP_CALLS) - 1 + N // HOP
    keys = keys_of(rows, 8200, dit=24, hand=HOP_HAND, burst=HOP_BURST + N // HOP, words_from=300)
    s, _, bins = gen.keyed_band(N, RATE, keys, 8250, hop=HOP, lead=0)
    s = s.copy()
    s[:HOP_BURST * HOP] *= np.float32(BURST_GAIN)
    return s, None, bins


def overlapped(origin):
    b = hop_band()
    return Case(N, 1, None, 0, [("batch", x) for x in HOP_CALLS], 8200, rate=RATE, bands=[b], init_bins=[b[2]], hop=HOP, trace=True,
                first_frame=origin)


def reports_rows(origin):
    """Reports and rows on: a batch in front, the deferred batch that straddles the crossing with a listener bound inside
    it on either side, a batch behind."""
    b = band()
    c = crossing(origin)
    late = [(0, b[2][1], c - 5), (0, b[2][2], c + 7)]
    steps = [("batch", DEFER[0]), ("defer", DEFER[1] - DEFER[0], late), ("batch", 170), ("batch", FRAMES - DEFER[1] - 170)]
    return Case(N, 1, None, 0, steps, 8100, rate=RATE, bands=[b], init_bins=[[b[2][0], b[2][3], b[2][4], b[2][5]]], first_frame=origin)


def traced(origin):
    """The bank's last batch straddles the crossing and completes the cumulations at frames 99 and 199; carrier 1's listener
    is bound inside it, ten frames behind the crossing."""
    b = band()
    b = (np.ascontiguousarray(b[0][:DEFER[1]]), None, b[2])
    late = [(0, b[2][1], crossing(origin) + 10)]
    steps = [("batch", DEFER[0]), ("defer", DEFER[1] - DEFER[0], late)]
    return Case(N, 1, None, 0, steps, 8100, rate=RATE, bands=[b], init_bins=[[b[2][0]] + b[2][2:]], trace=True, first_frame=origin)


GROUP_STEPS = (96, 1, 151, 52)


def grouped(origin):
    """Two bands for a group of two members on one device; the crossing on a batch boundary and inside the run."""
    bands = [band(N, RATE, 8100 + 7 * k) for k in range(2)]
    bands = [(np.ascontiguousarray(b[0][:sum(GROUP_STEPS)]), None, b[2]) for b in bands]
    return Case(N, 2, None, 0, [("batch", x) for x in GROUP_STEPS], 8100, rate=RATE, bands=bands, init_bins=[b[2] for b in bands],
                first_frame=origin)


# every case that crosses: (name, the Case) - the reach test walks this table, the GPU tests build the same cases
def crossing_cases():
    for origin in ORIGINS:
        for where in ("on", "in"):
            for debounce in (1, 5):
                yield f"eager-{origin}-{where}-d{debounce}", eager(origin, where, debounce)
    for origin in (O31, O32):
        yield f"attach_detach-{origin}", attach_detach(origin)
    yield f"stop-{O32}", stop(O32)
    yield f"deferred-{O31}", deferred(O31)
    yield f"deferred-wide-{O32}", deferred(O32, wide=True)
    for sc16 in (False, True):
        yield f"graph-{O32}-{'sc16' if sc16 else 'f32'}", graph(O32, sc16)
    yield f"overlapped-{O32}", overlapped(O32)
    for origin in (O31, O32):
        yield f"reports_rows-{origin}", reports_rows(origin)
    yield f"traced-{O5}", traced(O5)
    yield f"grouped-{O32}", grouped(O32)
