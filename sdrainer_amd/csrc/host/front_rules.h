// front_rules.h — the integer rules the front-end objects share (down-converter, channelizer, fine converter, blanker; the
// chain for its alignment): an object's sample clock and what a process call's length, pointers and strides must satisfy.
// Pure C++ without HIP, in the idiom of chain_plan.h: a rule returns an enum or a bool, the capi file that asks owns the text
// (csrc/front.h joins the two).  tests/host/test_front_rules.cpp drives every rule at its edges and tests/test_front_rules.py
// restates them.
#pragma once
#include <cstddef>
#include <cstdint>

namespace sdr {

// Sample indices of one object: `unit` is what a call's length and the first sample must be a multiple of (the decimation,
// or the blanker's block), max_in the most one call takes.
struct SampleClock {
    int64_t unit = 1, max_in = 0;
    int64_t origin = 0;    // index of the object's first sample
    int64_t total = 0;     // index of the next sample
    bool started = false;  // a process call has been accepted

    enum Refusal { Ok = 0, State, BadArg, BadSize };

    // before the first accepted call only: the next sample gets index k0
    Refusal set_first(int64_t k0)
    {
        if (started)
            return State;
        if (k0 < 0 || k0 % unit != 0)
            return BadArg;
        origin = total = k0;
        return Ok;
    }
    // a call's length: a positive multiple of the unit, at most max_in
    Refusal check_len(size_t n) const { return n == 0 || n % (size_t)unit != 0 || n > (size_t)max_in ? BadSize : Ok; }
    // behind a call whose kernels have been enqueued
    void advance(size_t n)
    {
        total += (int64_t)n;
        started = true;
    }
    // the blanker: how many of a call's first blocks still have fewer than `window` blocks behind them
    int warm_blocks(int window) const
    {
        const int64_t behind = (total - origin) / unit;
        return behind >= window ? 0 : (int)(window - behind);
    }
};

inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// the samples from one stream to the next in a buffer of several: a multiple of 4 and at least one stream's samples
inline bool stride_ok(size_t stride, size_t outputs) { return stride % 4 == 0 && stride >= outputs; }

// The bytes of n samples.  n is at most an object's max_in_samples, an int32, and a sample has at most 8 bytes: the product
// stays below 2^34 and cannot wrap a 64-bit size_t.
static_assert(sizeof(size_t) >= 8, "sample_bytes * n_in_samples must not wrap");
inline size_t span_bytes(int sample_bytes, size_t n) { return (size_t)sample_bytes * n; }

// [a, a + bytes) and [b, b + bytes) share a byte.  The distance of the two starts is compared, so nothing is added to an
// address and nothing wraps, wherever the ranges lie.
inline bool ranges_overlap(const void *a, const void *b, size_t bytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return (x < y ? y - x : x - y) < bytes;
}

inline bool step_valid(int step) { return step >= -32768 && step <= 32767; }  // an NCO step is an int16

}  // namespace sdr
