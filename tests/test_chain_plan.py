"""The receive chain's plan without a GPU: csrc/host/chain_plan.h, driven by the stand-alone program
tests/host/test_chain_plan.cpp (its own main, built with -fsanitize=address,undefined, the sanitizers' runtimes linked into
the program), against tests/chain_ref.py - every action of 160 seeded geometries and 48 pushes each, line for line - and the
invariants on that trace: even pointer offsets, carry moves that never overlap, nothing written past the ring, fewer than
block_size samples unconsumed after a piece, processed + pending == accepted.  Then sdr_chain_granule and sdr_chain_min_ring
through ctypes against the same restatement, refusals included."""
import os
import subprocess

import pytest

import chain_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_chain_plan.cpp")


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("chain_plan") / "test_chain_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    return p.stdout.splitlines()


@pytest.fixture(scope="module")
def restated():
    return CR.trace()


def test_the_trace_equals_the_restatement_line_for_line(printed, restated):
    lines, _ = restated
    assert len(printed) == len(lines)
    for i, (got, want) in enumerate(zip(printed, lines)):
        assert got == want, (i, got, want)


def test_the_cases_span_what_they_should(restated):
    _, cases = restated
    geos = [g for g, _ in cases]
    assert {g["block_size"] for g in geos} == {512, 1024, 2048, 4096, 8192}
    assert {g["block_size"] // g["hop"] for g in geos} == {1, 2, 4, 8, 16}
    dtots = {g["total_decimation"] for g in geos}
    assert 1 in dtots and 8192 in dtots and any(d & (d - 1) for d in dtots)
    assert {g["nb_block"] for g in geos} == set(CR.NB_BLOCKS) and 96 in CR.NB_BLOCKS
    # a granule that is a true lcm, pushes of one sample, of the whole capacity and of more than a piece
    assert any(CR.granule(g["total_decimation"], g["nb_block"]) not in (2 * g["total_decimation"], g["nb_block"], 16) for g in geos)
    pushes = [(g, n) for g, log in cases for n, _, _, _ in log]
    assert any(n == 1 for _, n in pushes) and any(n == g["max_in"] for g, n in pushes)
    assert any(n > CR.piece(CR.granule(g["total_decimation"], g["nb_block"]), g["limit"]) for g, n in pushes)


def test_invariants_of_the_printed_trace(printed):
    seen = CR.check_invariants(CR.parse(printed))
    # the trace exercises every action: thousands of pieces and batches, hundreds of carry moves and pending moves
    assert seen["piece"] > 2000 and seen["batch"] > 2000 and seen["move"] > 300 and seen["keep"] > 1000, seen
    assert "refuse size" in printed and "refuse state" in printed


def test_the_invariant_checker_notices_a_shifted_action(printed):
    """The checker is not vacuous: a batch one hop early, a carry move one sample short and a piece two samples late fail it."""
    cases = CR.parse(printed)
    for op, change in (("batch", lambda a: (a[0], a[1] - 2, a[2])), ("move", lambda a: (a[0], a[1], a[2], a[3] - 1)),
                       ("piece", lambda a: (a[0], a[1], a[2], a[3] + 2))):
        geo, log = next((g, lg) for g, lg in cases if any(a[0] == op for _, _, acts, _ in lg for a in acts))
        broken, done = [], False
        for n, host, acts, state in log:
            acts = list(acts)
            for i, a in enumerate(acts):
                if a[0] == op and not done:
                    acts[i], done = change(a), True
            broken.append((n, host, acts, state))
        with pytest.raises(AssertionError):
            CR.check_invariants([(geo, broken)])


@pytest.fixture(scope="module")
def capi():
    from sdrainer_amd.csrc import build
    build.build()
    from sdrainer_amd import capi as c
    return c


def test_granule_and_min_ring_through_ctypes(capi):
    for dtot in (1, 2, 3, 5, 32, 100, 1000, 8192, 65536):
        for nb in (1, 64, 96, 256, 4096):
            g = capi.chain_granule(dtot, nb)
            assert g == CR.granule(dtot, nb) and g % (2 * dtot) == 0 and g % nb == 0 and g % 16 == 0
            for block, hop in ((512, 128), (512, 512), (8192, 512), (65536, 4096)):
                for k in (1, 3):
                    assert capi.chain_min_ring(block, hop, k * g, dtot) == CR.min_ring(block, hop, k * g, dtot) >= 2 * block + k * g // dtot
    assert capi.chain_granule(32, 96) == 192 and capi.chain_granule(1, 1) == 16 and capi.chain_min_ring(512, 128, 64, 32) == 1028
    for dtot, nb in ((0, 1), (4, 0), (-2, 64), (4, -64)):
        assert capi.chain_granule(dtot, nb) < 0 and CR.granule(dtot, nb) < 0
    for args in ((0, 128, 4096, 32), (512, 0, 4096, 32), (512, 128, 0, 32), (512, 128, 4096, 0), (-512, 128, 4096, 32),
                 (512, -128, 4096, 32), (512, 128, -4096, 32), (512, 128, 4096, -32), (512, 1024, 4096, 32), (512, 128, 4097, 32)):
        assert capi.chain_min_ring(*args) < 0 and CR.min_ring(*args) < 0, args
