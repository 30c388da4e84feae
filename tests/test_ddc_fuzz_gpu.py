"""Seeded fuzz of the down-converter on the GPU (sdr_ddc_*, csrc/k_ddc.hip) against tests/ddc_ref.py, bit for bit: what
tests/ddc_fuzz_gen.py draws - every one of the kernel's nine tile shapes with every input format, 1 to 64 bands, the
steps at their ends, first samples that put 2^31 or 2^32 inside the run, streams of the formats' whole range, of zeros,
of full-scale runs and (float32) of Inf, NaN, +-FLT_MAX and -0 - run once as one call and once along the seed's cuts, the
cut run with device and host calls mixed, the host arrays overwritten as soon as a call returns, a retune and a move to a
second stream in front of a call.  tests/test_ddc_fuzz_coverage.py proves, without a GPU, what the default seeds reach.
A longer soak: SDR_DDC_FUZZ_SEEDS=400."""
import os

import numpy as np
import pytest

import ddc_fuzz_gen as gen
import parity_tools
from ddc_run import run_gpu
from parity_tools import capi  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def table(capi):
    return capi.ddc_nco_table()


@pytest.mark.parametrize("seed", gen.seeds(int(os.environ.get("SDR_DDC_FUZZ_SEEDS", gen.DEFAULT_SEEDS))), ids=lambda s: s.ident)
def test_seed(capi, table, seed):
    s = seed
    assert capi.DDC_TILE_OUTPUTS == gen.TILE
    same = getattr(parity_tools, s.same())
    raw, taps = s.raw(), s.taps()
    want_whole, want_cut = s.reference(*table, raw=raw)

    whole = run_gpu(capi, s.fmt, s.d, taps, s.steps, [raw], first_sample=s.first, host=s.whole_entry == "host")
    assert whole.shape == want_whole.shape == (s.n_bands, s.outputs, 2)
    assert same(whole, want_whole), f"{s.ident}: the whole stream in one call, {mismatch(whole, want_whole)}"

    retune = (lambda ddc, i: i == s.retune[0] and ddc.set_nco_step(*s.retune[1:])) if s.retune else None
    cut = run_gpu(capi, s.fmt, s.d, taps, s.steps, s.pieces(raw), first_sample=s.first, between=retune,
                  host=[e == "host" for e in s.entries], switch_at=s.switch_at)
    assert same(cut, want_cut), f"{s.ident}: along the cuts {s.cuts} ({s.entries}), {mismatch(cut, want_cut)}"


def mismatch(got, want):
    """Where two results differ: per band the number of differing outputs and the first of them."""
    bad = ((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).any(axis=2)
    return "; ".join(f"band {b}: {int(r.sum())} outputs from {int(np.argmax(r))}" for b, r in enumerate(bad) if r.any())
