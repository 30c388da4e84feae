"""Every named case of tests/peak_shape_gen.py is what its name says, on the oracle alone (no GPU): the peak list of every
cumulation tests/test_peak_shape_gpu.py compares holds exactly the designed runs with the designated maxima, the tied
case's pairs are tied bit for bit with the first bin reported, the capacity cases hold more runs than the max_peaks their
rows use (the exact-fit row exactly as many), and the edge row makes more edges in its long batch than a batch stores.  A
case the oracle does not confirm is a generator bug: nothing here is to be skipped or weakened to fit."""
import functools

import numpy as np
import pytest

import peak_shape_gen as gen
from oracle import oracle as orc
from sdrainer_amd import synth


@functools.lru_cache(maxsize=None)
def oracle_peaks(key, threshold):
    """(peak lists, cumulation rows) of one band's whole stream (the peak lists do not depend on batch cuts)."""
    n = key[0]
    r = orc.Receiver(gen.RATES[n], n, synth.default_edge_width(n), threshold, 1)
    out = r.process(gen._frames(key), max_peaks=4096)
    return out["peaks"], out["cumulation"]


BANDS = {(b.key, b.threshold): (row.id, b) for row in gen.ROWS for b in row.bands}


@pytest.mark.parametrize("key", sorted(BANDS, key=str), ids=lambda k: BANDS[k][0])
def test_the_oracle_finds_the_designed_runs(key):
    _, band = BANDS[key]
    peaks, cum = oracle_peaks(band.key, band.threshold)
    assert len(peaks) == band.frames // 100 >= 2
    for c, pk in enumerate(peaks):
        assert [(p[0], p[1], p[6]) for p in pk] == band.expected(c), f"cumulation {c}"
        if band.kind == "tied":
            row = cum[c].view(np.uint32)
            for a, e, m in band.expected(c):
                assert m == a and np.all(row[a:e + 1] == row[a]), f"cumulation {c}: the pair at {a} is not tied"
            assert sum(e > a for a, e, _ in band.expected(c)) == band.n // 4 - 1


def test_the_geometry_table_is_complete():
    """Every line of the table in tests/test_peak_shape_gpu.py's docstring is in some case, at every N that has the edge."""
    for n in (512, 8192, 16384, 32768):
        runs = {c: gen.geometry_runs(n, c) for c in ("abcd" if gen.spans(n) else "abc")}
        every = [r for rs in runs.values() for r in rs]
        w = gen.WORD
        for want in [(0, 2, 0), (n - 7, n - 1, n - 1), (0, 0, 0), (n - 1, n - 1, n - 1), (w - 2, w + 1, w), (63, 63, 63), (65, 65, 65)]:
            assert want in every, (n, want)
        assert any(a == e and a % w == w - 1 and a != 63 for a, e, _ in every) and any(a == e and a % w == 0 and a > 0 for a, e, _ in every)
        assert any(a % w == w - 2 and e == a + 3 and m == a + 1 for a, e, m in every)  # the maximum in front of the word end
        assert any(-(-a // w) * w + 2 * w - 1 <= e and e < n - 1 for a, e, _ in every), "no run over two whole words"
        assert any(e == n - 1 and m == a and a % w not in (0, w - 1) and (n - a) >= 3 * w for a, e, m in every), "no long open run"
        for s in gen.spans(n):
            for want in [(s - 2, s + 1, s - 1), (s - 2, s + 1, s), (s - 1, s - 1, s - 1), (s, s, s)]:
                assert want in every, (n, want)
    ids = [r.id for r in gen.ROWS]
    assert len(set(ids)) == len(ids)
    assert all(2 <= r.cumulations <= 4 for r in gen.ROWS)


def test_the_capacity_rows_overflow_and_the_exact_fit_row_fits():
    for row in gen.CAPACITY + [gen.GROUP]:
        counts = [len(pk) for b in row.bands for pk in oracle_peaks(b.key, b.threshold)[0]]
        assert counts == [x for i in range(len(row.bands)) for x in row.counts(i)]
        if row.id == gen.EXACT_FIT:
            assert all(c == row.max_peaks == 129 for c in counts)
        else:
            assert max(counts) > row.max_peaks, row.id
    for row in gen.CAPACITY[3:] + [gen.GROUP]:  # both conditions, in one batch where the row is one batch
        counts = row.counts(0)
        assert counts[0] > row.max_peaks and all(0 < c < row.max_peaks for c in counts[1:]) and len(counts) >= 3
    assert gen.CAPACITY[4].batches == [330] and gen.GROUP.batches == [330]
    for row in gen.GEOMETRY + gen.LISTENERS:  # (no geometry row is truncated by accident)
        assert all(max(row.counts(i)) <= row.max_peaks for i in range(len(row.bands))), row.id


def test_the_edge_row_makes_more_edges_than_a_batch_stores():
    iq, b = gen.edge_stream()
    n = gen.EDGE_N
    r = orc.Receiver(gen.EDGE_RATE, n, synth.default_edge_width(n), 15.0, 1)
    r.attach(b)
    out = r.process(iq)
    deb = out["deb"][:, 0].astype(np.int8)
    edges = np.flatnonzero(np.diff(np.concatenate([[0], deb])))
    head = int(np.count_nonzero(edges < gen.EDGE_FRAMES))
    assert head > gen.EDGE_CAP, head
    assert 0 < np.count_nonzero(edges >= gen.EDGE_FRAMES) < gen.EDGE_TAIL  # the keyed tail: edges, and not one per frame
    text = r.text(0)
    assert 0 < len(text) < 2048 and "dl1abc" in text, text[-80:]  # (the text buffer of 2048 runes never fills)
