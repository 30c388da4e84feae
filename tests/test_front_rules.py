"""The rules the front-end objects share, without a GPU: csrc/host/front_rules.h, driven at its edges by the stand-alone program
tests/host/test_front_rules.cpp (its own main, built with -fsanitize=address,undefined, the sanitizers' runtimes linked into
the program), against the restatement below, written from the C ABI's words (include/sdrainer_hip.h) - line for line."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "test_front_rules.cpp")
OK, STATE, BAD_ARG, BAD_SIZE = range(4)  # SampleClock::Refusal
I64_MAX, PTR_MAX, I32_MAX, I32_MIN = 2 ** 63 - 1, 2 ** 64 - 1, 2 ** 31 - 1, -2 ** 31


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("front_rules") / "test_front_rules")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and not p.stderr, p.stderr[-2000:]
    return p.stdout.splitlines()


def first_sample(started, unit, k0):
    """sdr_*_set_first_sample: only before the first process call; k0 >= 0 and a multiple of the unit."""
    if started:
        return STATE
    return OK if k0 >= 0 and k0 % unit == 0 else BAD_ARG


def length(unit, max_in, n):
    """n_in_samples: a positive multiple of the unit, at most max_in_samples."""
    return OK if 0 < n <= max_in and n % unit == 0 else BAD_SIZE


def warm(window, blocks_behind):
    """The blanker judges a block only with `window` blocks behind it: the call's first blocks that have fewer."""
    return max(0, window - blocks_behind)


def restated():
    out = []
    for unit in (1, 3, 4, 64, 256, 4096):
        max_in, top = 16 * unit, I64_MAX // unit * unit
        for k0 in (-1, 0, unit, unit + 1, top):
            rc = first_sample(False, unit, k0)
            at = k0 if rc == OK else 0
            out.append(f"set_first unit={unit} k0={k0} -> {rc} origin={at} total={at}")
            if k0 == top:
                continue
            out.append(f"set_first_started unit={unit} k0={k0} -> {first_sample(True, unit, max(k0, 0))} origin={at} total={at + unit} moved=0")
        for n in (0, unit, unit + 1, max_in, max_in + unit):
            out.append(f"check_len unit={unit} max_in={max_in} n={n} -> {length(unit, max_in, n)}")
        for call in range(6):
            out.append(f"warm_blocks unit={unit} behind={2 * call} -> {warm(1, 2 * call)} {warm(4, 2 * call)} {warm(64, 2 * call)}")
    for outputs in (1, 2, 3, 4, 5, 7, 8, 13, 510, 512):
        up = -(-outputs // 4) * 4
        for stride in (outputs - 1, outputs, up, up + 2, up + 4, 0):
            out.append(f"stride_ok stride={stride} outputs={outputs} -> {int(stride % 4 == 0 and stride >= outputs)}")
    most = 8 * I32_MAX
    out.append(f"span_bytes -> {most} 64 0")
    for nbytes in (1, 16, 4096, most):
        for a in (1 << 20, 1 << 40, PTR_MAX - 2 * nbytes - 1):
            for b in (a + nbytes + 1, a + nbytes, a + nbytes - 1, a, a + nbytes // 2, a + 1):
                assert b + nbytes - 1 <= PTR_MAX  # (every range lies inside the address space)
                # written out for the small sizes: some byte of one range is a byte of the other
                if nbytes <= 4096:
                    hit = bool(set(range(a, a + nbytes)) & set(range(b, b + nbytes)))
                else:
                    hit = a < b + nbytes and b < a + nbytes  # (Python's integers do not wrap)
                out.append(f"ranges_overlap a={a} b={b} bytes={nbytes} -> {int(hit)} {int(hit)}")
    out.append("ranges_overlap_empty -> 0")
    for p in (0, 1, 8, 15, 16, 4096 + 2, PTR_MAX - 15, PTR_MAX):
        out.append(f"aligned16 p={p} -> {int(p % 16 == 0)}")
    for step in (-32769, -32768, -1, 0, 32767, 32768, I32_MAX, I32_MIN):
        out.append(f"step_valid step={step} -> {int(-2 ** 15 <= step < 2 ** 15)}")
    return out


def test_the_rules_equal_the_restatement_line_for_line(printed):
    want = restated()
    assert len(printed) == len(want)
    for i, (got, line) in enumerate(zip(printed, want)):
        assert got == line, (i, got, line)


def test_the_edges_are_the_ones_that_matter(printed):
    """Every answer occurs, the doubly-wrong first sample reports the state, and the ranges at the top of the address space with
    the largest span a call can have are judged like the ones below."""
    text = "\n".join(printed)
    for rule, answers in (("set_first ", "02"), ("check_len ", "03"), ("stride_ok ", "01"), ("aligned16 ", "01"), ("step_valid ", "01")):
        assert {ln.split(" -> ")[1][0] for ln in printed if ln.startswith(rule)} == set(answers), rule
    assert all(" -> 1 " in ln for ln in printed if ln.startswith("set_first_started "))
    top = [ln for ln in printed if ln.startswith("ranges_overlap a=") and f"bytes={8 * I32_MAX} " in ln and f"a={PTR_MAX - 16 * I32_MAX - 1} " in ln]
    assert [ln.split(" -> ")[1] for ln in top] == ["0 0", "0 0", "1 1", "1 1", "1 1", "1 1"]
    assert f"set_first unit=4096 k0={I64_MAX // 4096 * 4096} -> 0" in text and "step_valid step=32768 -> 0" in text
