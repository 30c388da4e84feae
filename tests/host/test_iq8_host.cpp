// The 8-bit input path's host-checkable parts (sdrainer_amd/csrc/iq8.h), compiled with g++ -ffp-contract=off like the
// library's device code:
//   * both conversions (cs8, cu8) for all 256 inputs against the exact rationals x / 128 and (2 x - 255) / 256, in
//     float64, exact equality;
//   * k_fft_psd_iq8's staging image for N = 512 ... 16384: a bijection of the frame onto N*2 bytes, every DMA row reads
//     exactly its own 1 KB of the frame, every register slot of every thread reads the sample pass 0 wants there;
//   * the bank audit: the 32 lanes of each half of a wave's 16-bit read touch dwords that are equal or lie in different
//     banks (32 banks of four bytes; the two halves of one dword are served together).
// Prints "cs8:" and "cu8:" with the 256 values each (hex floats) and "ok".
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sdrainer_amd/csrc/iq8.h"

template <int LOGN>
static int audit_image()
{
    using PL = fft64::Plan<LOGN>;
    constexpr int N = PL::N;
    int bad = 0;
    // image: a bijection onto [0, 2N), 2-byte aligned
    std::vector<int> owner(N, -1);
    for (int n = 0; n < N; n++) {
        const int a = iq8::lds_byte<LOGN>(n);
        if (a < 0 || a >= 2 * N || (a & 1) || owner[a / 2] >= 0) {
            std::printf("N=%d: sample %d -> byte %d (bad or taken)\n", N, n, a);
            return 1;
        }
        owner[a / 2] = n;
    }
    // DMA: lane p of row r writes row base + 16 p from source granule g = granule(p, r) of the row; wave w of the workgroup
    // fetches rows w * kRowsPerWave ... and the waves' rows are the frame's
    if (iq8::kRowsPerWave<LOGN> * (PL::T / 64) != iq8::kRows<LOGN> || iq8::kRows<LOGN> * 1024 != 2 * N) {
        std::printf("N=%d: %d waves x %d rows do not cover %d rows\n", N, PL::T / 64, iq8::kRowsPerWave<LOGN>, iq8::kRows<LOGN>);
        return 1;
    }
    for (int r = 0; r < iq8::kRows<LOGN>; r++) {
        std::vector<int> seen(64, 0);
        for (int p = 0; p < 64; p++) {
            const int g = iq8::granule<LOGN>(p, r);
            if (g < 0 || g >= 64 || seen[g]++) {
                std::printf("N=%d row %d: lane %d fetches granule %d (bad or twice)\n", N, r, p, g);
                return 1;
            }
            for (int i = 0; i < 8; i++)
                if (iq8::lds_byte<LOGN>(r * 512 + g * 8 + i) != r * 1024 + p * 16 + 2 * i)
                    bad++;
        }
    }
    // reads: thread part XOR slot part = the sample's address; dwords and banks of each 32-lane group
    int worst = 1;
    for (int m = 0; m < PL::R; m++) {
        const int slot_byte = iq8::lds_byte<LOGN>(fft64::input_sample<LOGN>(0, m));
        for (int t0 = 0; t0 < PL::T; t0 += 32) {
            int dword_of_bank[32];
            int degree[32] = {};
            for (int k = 0; k < 32; k++)
                dword_of_bank[k] = -1;
            for (int t = t0; t < t0 + 32; t++) {
                const int n = fft64::input_sample<LOGN>(t, m);
                const int a = iq8::lds_byte<LOGN>(fft64::input_sample<LOGN>(t, 0)) ^ slot_byte;
                if (a != iq8::lds_byte<LOGN>(n))
                    bad++;
                const int dw = a / 4, bank = dw % 32;
                if (dword_of_bank[bank] != dw) {  // (another dword of the same bank: one more cycle)
                    dword_of_bank[bank] = dw;
                    degree[bank]++;
                }
            }
            for (int k = 0; k < 32; k++)
                if (degree[k] > worst)
                    worst = degree[k];
        }
    }
    if (worst != 1) {
        std::printf("N=%d: bank conflict of degree %d\n", N, worst);
        return 1;
    }
    if (bad)
        std::printf("N=%d: %d address mismatches\n", N, bad);
    return bad != 0;
}

int main()
{
    const iq8::Format cs8 = iq8::format_of(false), cu8 = iq8::format_of(true);
    int wrong = 0;
    std::printf("cs8:");
    for (int v = -128; v <= 127; v++) {
        const uint32_t w = (uint32_t)(uint8_t)(int8_t)v;
        // the byte in the I place with another byte beside it, and in the Q place
        const float re = iq8::re_of(w | 0x5a00u, cs8), im = iq8::im_of((w << 8) | 0xa5u, cs8);
        const double want = (double)v / 128.0;
        if ((double)re != want || (double)im != want)
            wrong++;
        std::printf(" %a", re);
    }
    std::printf("\ncu8:");
    for (int v = 0; v <= 255; v++) {
        const uint32_t w = (uint32_t)v;
        const float re = iq8::re_of(w | 0x5a00u, cu8), im = iq8::im_of((w << 8) | 0xa5u, cu8);
        const double want = (2.0 * v - 255.0) / 256.0;
        if ((double)re != want || (double)im != want)
            wrong++;
        std::printf(" %a", re);
    }
    std::printf("\n");
    if (wrong) {
        std::printf("conversion wrong for %d inputs\n", wrong);
        return 1;
    }
    if (audit_image<9>() | audit_image<10>() | audit_image<11>() | audit_image<12>() | audit_image<13>() | audit_image<14>())
        return 1;
    std::printf("ok\n");
    return 0;
}
