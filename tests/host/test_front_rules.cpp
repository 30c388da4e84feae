// test_front_rules.cpp — csrc/host/front_rules.h at its edges, as a stand-alone program (built by tests/test_front_rules.py with
// -fsanitize=address,undefined): one line per question, which the Python test compares with its own restatement of the rules.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../sdrainer_amd/csrc/host/front_rules.h"

using sdr::SampleClock;

static const void *at(uintptr_t a) { return reinterpret_cast<const void *>(a); }

int main()
{
    const int64_t units[] = {1, 3, 4, 64, 256, 4096};
    for (int64_t unit : units) {
        const int64_t max_in = 16 * unit, top = INT64_MAX / unit * unit;
        const int64_t firsts[] = {-1, 0, unit, unit + 1, top};
        for (int64_t k0 : firsts) {
            SampleClock c;
            c.unit = unit;
            c.max_in = max_in;
            const int fresh = c.set_first(k0);
            printf("set_first unit=%" PRId64 " k0=%" PRId64 " -> %d origin=%" PRId64 " total=%" PRId64 "\n", unit, k0, fresh, c.origin, c.total);
            if (k0 == top)
                continue;  // (a call behind the last representable sample is nobody's stream)
            c.advance((size_t)unit);
            const int64_t total = c.total;
            const int late = c.set_first(k0 < 0 ? 0 : k0);
            printf("set_first_started unit=%" PRId64 " k0=%" PRId64 " -> %d origin=%" PRId64 " total=%" PRId64 " moved=%d\n", unit, k0, late,
                   c.origin, c.total, (int)(c.total != total));
        }
        SampleClock c;
        c.unit = unit;
        c.max_in = max_in;
        const int64_t lens[] = {0, unit, unit + 1, max_in, max_in + unit};
        for (int64_t n : lens)
            printf("check_len unit=%" PRId64 " max_in=%" PRId64 " n=%" PRId64 " -> %d\n", unit, max_in, n, (int)c.check_len((size_t)n));
        // the blanker's warm-up over the first calls of a stream that starts at 5 units
        c.set_first(5 * unit);
        for (int call = 0; call < 6; call++) {
            printf("warm_blocks unit=%" PRId64 " behind=%d -> %d %d %d\n", unit, 2 * call, c.warm_blocks(1), c.warm_blocks(4), c.warm_blocks(64));
            c.advance((size_t)(2 * unit));
        }
    }
    for (size_t outputs : {1u, 2u, 3u, 4u, 5u, 7u, 8u, 13u, 510u, 512u}) {
        const size_t up = (outputs + 3) / 4 * 4;
        for (size_t stride : {outputs - 1, outputs, up, up + 2, up + 4, (size_t)0})
            printf("stride_ok stride=%zu outputs=%zu -> %d\n", stride, outputs, (int)sdr::stride_ok(stride, outputs));
    }
    // ranges of `bytes` each: far apart, adjacent, sharing one byte, identical, one starting inside the other, either way round
    const size_t most = sdr::span_bytes(8, (size_t)INT32_MAX);  // the largest a call can span: 8-byte samples, max_in_samples at its limit
    printf("span_bytes -> %zu %zu %zu\n", most, sdr::span_bytes(1, 64), sdr::span_bytes(2, 0));
    for (size_t bytes : {(size_t)1, (size_t)16, (size_t)4096, most}) {
        const uintptr_t bases[] = {(uintptr_t)1 << 20, (uintptr_t)1 << 40, UINTPTR_MAX - 2 * bytes - 1};  // the last: b's range ends at the top
        for (uintptr_t a : bases) {
            const uintptr_t others[] = {a + bytes + 1, a + bytes, a + bytes - 1, a, a + bytes / 2, a + 1};
            for (uintptr_t b : others)
                printf("ranges_overlap a=%" PRIuPTR " b=%" PRIuPTR " bytes=%zu -> %d %d\n", a, b, bytes, (int)sdr::ranges_overlap(at(a), at(b), bytes),
                       (int)sdr::ranges_overlap(at(b), at(a), bytes));
        }
    }
    printf("ranges_overlap_empty -> %d\n", (int)sdr::ranges_overlap(at(64), at(64), 0));
    for (uintptr_t p : {(uintptr_t)0, (uintptr_t)1, (uintptr_t)8, (uintptr_t)15, (uintptr_t)16, (uintptr_t)4096 + 2, UINTPTR_MAX - 15, UINTPTR_MAX})
        printf("aligned16 p=%" PRIuPTR " -> %d\n", p, (int)sdr::aligned16(at(p)));
    for (int step : {-32769, -32768, -1, 0, 32767, 32768, INT32_MAX, INT32_MIN})
        printf("step_valid step=%d -> %d\n", step, (int)sdr::step_valid(step));
    return 0;
}
