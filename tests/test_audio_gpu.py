"""The Goertzel audio path (sdr_audio_*, csrc/sdr_audio.hip) beyond one stream, one rate and one scale, bit for bit against
oracle.AudioDemodulator, one instance per stream.

Every case goes through one driver (run): a bank and one oracle per stream receive the same setters at the same sample
positions and the same ragged writes (tests/audio_gen.py cuts); after EVERY write EVERY stream's trace of that write -
normalised magnitudes bit for bit (any NaN equals any NaN), raw and debounced states, the block count - is compared, and
the text: streams with an even index are read after every write, the others at the end only.  tests/test_audio_host.py
holds the conditions that make each case what its name says."""
import ctypes as C

import numpy as np
import pytest

import audio_gen as gen
from oracle import oracle as orc
from parity_tools import capi, nan_equal_bits  # noqa: F401 (capi: the fixture)

pytestmark = pytest.mark.gpu

MAX_BLOCKS = 1024


def run(capi, case, sr, pitch, xs, scale=None, max_blocks=MAX_BLOCKS, cuts=None, before=None, blocksize=None):
    """xs: one float32 array per stream, of equal length.  before: {write index: [(setter name, value), ...]}, applied to
    the bank and to every oracle ahead of that write.  Returns the oracles' texts."""
    n = len(xs)
    bank = capi.AudioBank(n, pitch, sr, max_blocks=max_blocks)
    refs = [orc.AudioDemodulator(pitch, sr) for _ in range(n)]
    bs = bank.blocksize
    assert bs == refs[0].blocksize, f"{case}: blocksize {bs}, the oracle's {refs[0].blocksize}"
    if blocksize is not None:
        assert bs == blocksize, f"{case}: blocksize {bs}, the table's {blocksize}"
    if scale is not None:
        bank.set_scale(scale)
        for r in refs:
            r.set_scale(scale)
    cuts = gen.cuts(xs[0].size, bs, max_blocks, n) if cuts is None else cuts
    before = before or {}
    text = [""] * n
    x = np.stack(xs)
    for w, (a, e) in enumerate(zip(cuts[:-1], cuts[1:])):
        for name, value in before.get(w, ()):
            getattr(bank, name)(value)
            for r in refs:
                getattr(r, name)(value)
        bank.write(x[:, a:e])
        want_blocks = e // bs - a // bs
        for s in range(n):
            where = f"{case} stream {s} write {w} [{a}, {e})"
            wm, wr, wd = refs[s].write(xs[s][a:e])
            assert len(wm) == want_blocks, f"{where}: the oracle completed {len(wm)} blocks, not {want_blocks}"
            m, r, d = bank.read_trace(s, max_blocks)
            assert len(m) == len(wm), f"{where}: {len(m)} blocks, the oracle's {len(wm)}"
            assert nan_equal_bits(m, wm), f"{where}: magnitudes differ first at block {first_difference(m, wm)}"
            assert np.array_equal(r, wr), f"{where}: raw states differ first at block {np.flatnonzero(r != wr)[:1]}"
            assert np.array_equal(d, wd), f"{where}: debounced states differ first at block {np.flatnonzero(d != wd)[:1]}"
            if s % 2 == 0:
                text[s] += bank.read_text(s)
                assert text[s] == refs[s].text(), f"{where}: text {text[s]!r}, the oracle's {refs[s].text()!r}"
    bank.close()
    for r in refs:
        r.close()
    for s in range(n):
        text[s] += bank.read_text(s)
        assert text[s] == refs[s].text(), f"{case} stream {s} at the end: text {text[s]!r}, the oracle's {refs[s].text()!r}"
        assert bank.read_text(s) == "", f"{case} stream {s}: text delivered twice"
    bank.close_handle()
    return text


def first_difference(a, b):
    both_nan = np.isnan(a) & np.isnan(b)
    return np.flatnonzero((a.view(np.uint64) != b.view(np.uint64)) & ~both_nan)[:1]


# -- many streams -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,pitch,n,scale", gen.MANY, ids=[f"{c[0]}-{c[2]}-{c[3]:g}" for c in gen.MANY])
def test_many_streams(capi, sr, pitch, n, scale):
    """130 = 64 + 64 + 2 streams (65; 1): every workgroup of k_audio_decode, a wave with two lanes, and lanes of one wave
    in different decoder states.  max_blocks = 1024 and streams of 2100 - 2900 blocks: several writes each."""
    xs = gen.streams(sr, pitch, n, gen.SEED)
    text = run(capi, f"{sr}/{pitch:g} x{n} scale {scale:g}", sr, pitch, xs, scale=scale)
    if n >= 64:
        assert len(set(text)) >= 20, "the streams' texts do not differ"


# -- the remaining geometries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,pitch,bs", gen.SMALL_GEOMETRY, ids=[f"{g[0]}-{g[1]:g}" for g in gen.SMALL_GEOMETRY])
def test_geometry(capi, sr, pitch, bs):
    xs = gen.streams(sr, pitch, 3, gen.SEED)
    assert len({x.tobytes() for x in xs}) == 3
    run(capi, f"{sr}/{pitch:g}", sr, pitch, xs, scale=0.0, blocksize=bs)


@pytest.mark.parametrize("n,pitch,sr", [(2, 30.0, 8000), (2, 0.0, 8000), (2, float("nan"), 8000), (0, 600.0, 8000)],
                         ids=["blocksize0", "pitch0", "pitchnan", "streams0"])
def test_geometry_refused(capi, n, pitch, sr):
    with pytest.raises(capi.SdrError) as e:
        capi.AudioBank(n, pitch, sr, max_blocks=16)
    assert e.value.code == capi.ERR_BAD_ARG


# -- value regimes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", (0.0, 1.0), ids=["autoscale", "scale1"])
@pytest.mark.parametrize("name", gen.REGIMES)
def test_value_regime(capi, name, scale):
    """Subnormal samples, samples times 2^100 and 2^127, +Inf / -Inf / NaN and a block of -0.0 on streams 0, 2 and 3 of
    five; streams 1 and 4 stay ordinary (and are compared like the others)."""
    sr, pitch = gen.REGIME_GEOMETRY
    run(capi, f"{name} scale {scale:g}", sr, pitch, gen.regime_bank(name), scale=scale)


# -- setters during a stream -------------------------------------------------------------------------------------------
def test_setters_during_a_stream(capi):
    """70 streams: the round trip of the device state through the host (update_states) covers a second workgroup's
    streams.  Every setter falls between two writes, most of them with samples pending."""
    sr, pitch = gen.MANY_GEOMETRY[0]
    xs = gen.streams(sr, pitch, 70, gen.SEED)
    bs = gen.blocksize(sr, pitch)
    nb = xs[0].size // bs
    assert nb >= 2000
    step = nb // 8
    cuts = [0] + [k * step * bs + (7 * k) % bs for k in range(1, 8)] + [xs[0].size]
    assert sum(c % bs != 0 for c in cuts[1:-1]) >= 5
    before = {1: [("set_debounce", 1)], 2: [("set_magnitude_threshold", 0.5)], 3: [("set_scale", 0.0)],
              4: [("set_debounce", 5)], 5: [("set_magnitude_threshold", 0.9)], 6: [("set_scale", 2.5)],
              7: [("set_debounce", 1), ("set_magnitude_threshold", 0.5)]}
    run(capi, "setters", sr, pitch, xs, scale=1.0, cuts=cuts, before=before)


# -- the write contract ------------------------------------------------------------------------------------------------
def test_write_contract(capi):
    sr, pitch = gen.MANY_GEOMETRY[0]
    xs = gen.streams(sr, pitch, 3, gen.SEED)
    bs, mb = gen.blocksize(sr, pitch), 100
    x = np.stack(xs)
    assert x.shape[1] >= (3 * mb + 2) * bs
    bank = capi.AudioBank(3, pitch, sr, max_blocks=mb)
    refs = [orc.AudioDemodulator(pitch, sr) for _ in range(3)]

    def compare(a, e, what, blocks):
        for s in range(3):
            wm, wr, wd = refs[s].write(xs[s][a:e])
            m, r, d = bank.read_trace(s, mb)
            assert len(m) == len(wm) == blocks, f"{what} stream {s}: {len(m)} blocks, the oracle's {len(wm)}, expected {blocks}"
            assert nan_equal_bits(m, wm) and np.array_equal(r, wr) and np.array_equal(d, wd), f"{what} stream {s}: trace differs"

    # a write that completes no block: read_trace reports 0 blocks (not the blocks of the write before)
    bank.write(x[:, :bs + 5])
    compare(0, bs + 5, "first write", 1)
    bank.write(x[:, bs + 5:bs + 9])
    compare(bs + 5, bs + 9, "write that completes no block", 0)
    # exactly max_blocks blocks, the 9 pending samples included
    a, e = bs + 9, (mb + 1) * bs + 3
    bank.write(x[:, a:e])
    compare(a, e, "write of exactly max_blocks blocks", mb)
    # read_trace with max = 5: the first 5, and the full count
    want = bank.read_trace(1, mb)
    m, r, d, n = np.full(8, -1.0), np.full(8, 9, np.uint8), np.full(8, 9, np.uint8), C.c_int()
    rc = bank._L.sdr_audio_read_trace(bank._h, 1, C.c_void_p(m.ctypes.data), C.c_void_p(r.ctypes.data), C.c_void_p(d.ctypes.data), 5, C.byref(n))
    assert rc == 0 and n.value == mb, f"read_trace with max 5 reports {n.value} blocks, not {mb}"
    assert nan_equal_bits(m[:5], want[0][:5]) and np.array_equal(r[:5], want[1][:5]) and np.array_equal(d[:5], want[2][:5])
    assert np.all(m[5:] == -1) and np.all(r[5:] == 9) and np.all(d[5:] == 9), "read_trace wrote beyond max"
    # one block more than max_blocks is refused, and the refusal changes nothing: the same samples in two halves then
    # give what the oracle gives
    a, e = e, e + (mb + 1) * bs - 3
    assert (e // bs) - (a // bs) == mb + 1
    with pytest.raises(capi.SdrError) as err:
        bank.write(x[:, a:e])
    assert err.value.code == capi.ERR_WOULD_DROP
    half = a + (e - a) // 2
    bank.write(x[:, a:half])
    compare(a, half, "first half after the refusal", half // bs - a // bs)
    bank.write(x[:, half:e])
    compare(half, e, "second half after the refusal", e // bs - half // bs)
    # stream indices
    for s in (-1, 3):
        with pytest.raises(capi.SdrError) as err:
            bank.read_trace(s, mb)
        assert err.value.code == capi.ERR_BAD_ARG
        with pytest.raises(capi.SdrError) as err:
            bank.read_text(s)
        assert err.value.code == capi.ERR_BAD_ARG
    bank.close()
    for s in range(3):
        refs[s].close()
        assert bank.read_text(s) == refs[s].text(), f"stream {s}: text"
    bank.close_handle()


# -- text delivery -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def delivery():
    x, bs = gen.delivery_stream(gen.DELIVERY_BLOCKS_LONG)
    x.setflags(write=False)
    return x, bs, gen.delivery_oracle(x)


def delivery_bank(capi, max_blocks):
    sr, pitch = gen.DELIVERY_GEOMETRY
    bank = capi.AudioBank(1, pitch, sr, max_blocks=max_blocks)
    bank.set_debounce(1)
    return bank


def test_text_small_buffer_loses_nothing(capi, delivery):
    """sdr_audio_read_text with a 101-byte buffer, until it returns 0 bytes: 50 two-byte runes per call, never half a rune,
    and the concatenation is the oracle's text."""
    x, bs, _ = delivery
    x = x[:gen.DELIVERY_BLOCKS_SHORT * bs]
    want = gen.delivery_oracle(x)
    assert len(want) == 1875
    bank = delivery_bank(capi, gen.DELIVERY_BLOCKS_SHORT)
    bank.write(x[None, :])
    bank.close()
    buf, n, got, calls = C.create_string_buffer(101), C.c_int(), b"", 0
    while True:
        rc = bank._L.sdr_audio_read_text(bank._h, 0, buf, 101, C.byref(n))
        assert rc == 0
        calls += 1
        if n.value == 0:
            break
        assert n.value % 2 == 0 and n.value <= 100, f"call {calls}: {n.value} bytes split a rune"
        got += buf.raw[:n.value]
        assert calls <= len(want), "read_text never runs dry"
    assert got.decode("utf-8") == want, f"{len(got) // 2} runes delivered in {calls} calls, the oracle wrote {len(want)}"
    bank.close_handle()


def test_text_read_after_every_write(capi, delivery):
    x, bs, want = delivery
    bank = delivery_bank(capi, 16384)
    got = ""
    for a in range(0, x.size, 16000 * bs + 11):
        bank.write(x[None, a:a + 16000 * bs + 11])
        got += bank.read_text(0)
    bank.close()
    got += bank.read_text(0)
    assert len(want) > gen.TEXT_CAP and got == want, f"{len(got)} runes delivered, the oracle wrote {len(want)}"
    bank.close_handle()


def test_text_store_holds_4096_runes(capi, delivery):
    """Never read until the end: a stream stores its first 4096 undelivered runes and drops the later ones."""
    x, bs, want = delivery
    bank = delivery_bank(capi, 16384)
    for a in range(0, x.size, 16000 * bs + 11):
        bank.write(x[None, a:a + 16000 * bs + 11])
    bank.close()
    got = bank.read_text(0)
    assert len(want) > gen.TEXT_CAP and got == want[:gen.TEXT_CAP], f"{len(got)} runes delivered"
    assert bank.read_text(0) == ""
    bank.close_handle()
