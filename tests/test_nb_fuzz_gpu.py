"""Seeded fuzz of the impulse noise blanker on the GPU (sdr_nb_*, csrc/k_nb.hip) against tests/nb_ref.py, byte for byte and
with equal statistics at every read: what tests/nb_fuzz_gen.py draws - every integer format with every block size from 64 to
4096, so every bgl of both streaming kernels, W from 1 to 64, holds from 0 to B that stay inside a 16-byte group, loop in
the lookback in front of a tile, run down a wave's rows and across the waves, ratios from 16 to 16384, streams of whole-range
words, of noise with full-scale samples at every structure's ends, of one constant magnitude (the strict inequality at
equality) and of full-scale stretches (the saturated threshold), first samples above 2^32 - run once as one call and once
along the seed's cuts, there with device and host calls mixed, thresholds switched off and on, a long hold and a shorter
one while its gate is open, and the statistics read between calls.  tests/test_nb_fuzz_coverage.py proves, without a GPU,
what the default seeds reach.  A longer soak: SDR_NB_FUZZ_SEEDS=400."""
import os

import numpy as np
import pytest

import nb_fuzz_gen as gen
from nb_run import run_nb
from parity_tools import bits_equal, capi  # noqa: F401

pytestmark = pytest.mark.gpu


def first_difference(got, want):
    bad = (got != want).reshape(len(got), -1).any(axis=1)
    return f"{int(bad.sum())} samples differ, the first at {int(np.argmax(bad))}" if bad.any() else "dtype or shape"


@pytest.mark.parametrize("seed", gen.seeds(int(os.environ.get("SDR_NB_FUZZ_SEEDS", gen.DEFAULT_SEEDS))), ids=lambda s: s.ident)
def test_seed(capi, seed):
    s = seed
    assert capi.nb_tile_samples(s.fmt, s.B) == s.tile
    raw = s.raw()
    (want_whole, want_stats), (want_outs, want_reads) = s.reference(raw)

    (whole,), (stats,) = run_nb(capi, s.fmt, s.B, s.W, s.ratio_q4, s.hold, [raw], host=s.whole_entry == "host", first_sample=s.first)
    assert bits_equal(whole, want_whole), f"{s.ident}: the whole stream in one call, {first_difference(whole, want_whole)}"
    assert stats == want_stats, f"{s.ident}: the whole stream in one call"

    outs, reads = run_nb(capi, s.fmt, s.B, s.W, s.ratio_q4, s.hold, s.pieces(raw), host=[e == "host" for e in s.entries],
                         thresholds=s.thresholds, first_sample=s.first, reads=s.reads)
    what = f"{s.ident}: along the cuts {s.cuts} ({s.entries}, thresholds {s.thresholds})"
    assert len(outs) == len(want_outs)
    for i, (g, w) in enumerate(zip(outs, want_outs)):
        assert bits_equal(g, w), f"{what}, call {i}: {first_difference(g, w)}"
    assert reads == want_reads, what
