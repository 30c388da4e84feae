"""Seeded fuzz of the fine converter on the GPU (sdr_fine_*, csrc/k_fine.hip) against tests/fine_ref.py, bit for bit: what
tests/fine_fuzz_gen.py draws - every one of the kernel's nine tile shapes twice, 1 to 256 inputs and 1 to 64 bands with
several bands on one input and one input unread, the steps at their ends, first samples that put 2^31 or 2^32 inside the
run, inputs that lie back to back or a gap apart, streams of plain values, of signed zeros, of Inf, NaN, +-FLT_MAX and -0,
and of values whose every output is subnormal - run once as one call and once along the seed's cuts, there with a band moved
to an input nobody has read and back, a retune and a move to a second stream in front of a call.
tests/test_fine_fuzz_coverage.py proves, without a GPU, what the default seeds reach.  A longer soak:
SDR_FINE_FUZZ_SEEDS=200."""
import os

import numpy as np
import pytest

import fine_fuzz_gen as gen
import parity_tools
from fine_run import run_gpu
from parity_tools import capi  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


@pytest.mark.parametrize("seed", gen.seeds(int(os.environ.get("SDR_FINE_FUZZ_SEEDS", gen.DEFAULT_SEEDS))), ids=lambda s: s.ident)
def test_seed(capi, table, seed):
    s = seed
    assert capi.DDC_TILE_OUTPUTS == gen.TILE
    same = getattr(parity_tools, s.same())
    x, taps = s.streams(), s.taps()
    want_whole, want_cut = s.reference(*table, x=x)

    whole = run_gpu(capi, s.d, taps, s.steps, s.inputs, [x], first_sample=s.first, in_gap=s.gaps[0], out_gap=s.gaps[1])
    assert whole.shape == want_whole.shape == (s.n_bands, s.outputs, 2)
    assert same(whole, want_whole), f"{s.ident}: the whole streams in one call, inputs {s.inputs}, {mismatch(whole, want_whole)}"

    cut = run_gpu(capi, s.d, taps, s.steps, s.inputs, s.pieces(x), first_sample=s.first, between=s.between, switch_at=s.switch_at,
                  in_gap=s.gaps[2], out_gap=s.gaps[3])
    assert same(cut, want_cut), f"{s.ident}: along the cuts {s.cuts}, inputs {s.inputs}, changes {s.changes}, {mismatch(cut, want_cut)}"


def mismatch(got, want):
    """Where two results differ: per band the number of differing outputs and the first of them."""
    bad = ((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).any(axis=2)
    return "; ".join(f"band {b}: {int(r.sum())} outputs from {int(np.argmax(r))}" for b, r in enumerate(bad) if r.any())
