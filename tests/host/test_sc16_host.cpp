// The sc16 input path's host-checkable parts (sdrainer_amd/csrc/sc16.h), compiled with g++ -ffp-contract=off like the
// library's device code:
//   * the conversion against a correctly rounded division (float64 quotient, rounded once) for all 65 536 inputs;
//   * k_fft_psd_sc16's staging image for N = 512 ... 16384: a bijection of the frame onto N*4 bytes, every DMA row reads
//     exactly its own 1 KB of the frame, every register slot of every thread reads the sample pass 0 wants there, and
//     each 32-lane group of a ds_read_b32 touches 32 different banks.
// Prints "multiply-wrong: <values>" (the inputs where x * (1/32767) differs, for the GPU test's input) and "ok".
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sdrainer_amd/csrc/sc16.h"

static unsigned bits(float f)
{
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}

template <int LOGN>
static int audit_image()
{
    using PL = fft64::Plan<LOGN>;
    constexpr int N = PL::N;
    int bad = 0;
    // image: a bijection onto [0, 4N), word-aligned
    std::vector<int> owner(N, -1);
    for (int n = 0; n < N; n++) {
        const int a = sc16::lds_byte<LOGN>(n);
        if (a < 0 || a >= 4 * N || (a & 3) || owner[a / 4] >= 0) {
            std::printf("N=%d: sample %d -> byte %d (bad or taken)\n", N, n, a);
            return 1;
        }
        owner[a / 4] = n;
    }
    // DMA: lane p of row r writes row base + 16 p from source granule g = granule(p, r) of the row
    for (int r = 0; r < N / 256; r++) {
        std::vector<int> seen(64, 0);
        for (int p = 0; p < 64; p++) {
            const int g = sc16::granule<LOGN>(p, r);
            if (g < 0 || g >= 64 || seen[g]++) {
                std::printf("N=%d row %d: lane %d fetches granule %d (bad or twice)\n", N, r, p, g);
                return 1;
            }
            for (int i = 0; i < 4; i++)
                if (sc16::lds_byte<LOGN>(r * 256 + g * 4 + i) != r * 1024 + p * 16 + 4 * i)
                    bad++;
        }
    }
    // reads: thread part XOR slot part = the sample's address; banks of each 32-lane group
    for (int m = 0; m < PL::R; m++) {
        const int slot_byte = sc16::lds_byte<LOGN>(fft64::input_sample<LOGN>(0, m));
        for (int t0 = 0; t0 < PL::T; t0 += 32) {
            unsigned banks = 0;
            for (int t = t0; t < t0 + 32; t++) {
                const int n = fft64::input_sample<LOGN>(t, m);
                const int a = sc16::lds_byte<LOGN>(fft64::input_sample<LOGN>(t, 0)) ^ slot_byte;
                if (a != sc16::lds_byte<LOGN>(n))
                    bad++;
                banks |= 1u << ((a / 4) % 32);
            }
            if (banks != 0xffffffffu) {
                std::printf("N=%d slot %d threads %d..: bank conflict (mask %08x)\n", N, m, t0, banks);
                return 1;
            }
        }
    }
    if (bad)
        std::printf("N=%d: %d address mismatches\n", N, bad);
    return bad != 0;
}

int main()
{
    int wrong = 0;
    std::printf("multiply-wrong:");
    for (int v = -32768; v <= 32767; v++) {
        const float want = (float)((double)v / 32767.0);  // the double quotient is exact enough to round once
        const float got = sc16::to_f32((int16_t)v);
        if (bits(got) != bits(want)) {
            if (wrong++ < 8)
                std::fprintf(stderr, "to_f32(%d) = %a, want %a\n", v, got, want);
        }
        volatile float inv = 1.0f / 32767.0f;
        if (bits((float)v * inv) != bits(want))
            std::printf(" %d", v);
    }
    std::printf("\n");
    if (wrong) {
        std::printf("conversion wrong for %d inputs\n", wrong);
        return 1;
    }
    // the word helpers: I in the low half, Q in the high half
    if (bits(sc16::re_of(0x80017fffu)) != bits(1.0f) || bits(sc16::im_of(0x80017fffu)) != bits((float)(-32767.0 / 32767.0)))
        return 1;
    if (audit_image<9>() | audit_image<10>() | audit_image<11>() | audit_image<12>() | audit_image<13>() | audit_image<14>())
        return 1;
    std::printf("ok\n");
    return 0;
}
