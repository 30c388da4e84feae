// The audit of a one-frame FFT kernel's staging image (sdrainer_amd/csrc/fft_f64.h InImage: float32's, sc16.h's, iq8.h's),
// N = 2^LOGN, for the host programs of the formats:
//   * the image is a bijection of the frame's samples onto N * SAMPLE_BYTES bytes, aligned to the sample;
//   * the waves' rows are the frame's, and lane p of row r, which the DMA writes at row base + 16 p, fetches a granule of
//     that row's own 1 KB, each once, whose samples have exactly those addresses;
//   * every register slot of every thread reads the sample pass 0 wants there, its address the XOR of the thread's part
//     and the slot's constant;
//   * the banks: the 32 lanes of each half of a wave's read touch words (four bytes, eight for the 64-bit reads of the
//     float32 image) that are equal or lie in different banks - 16-bit reads of the two halves of one dword are served
//     together - and reads of at least a dword, which cannot share one, therefore touch all 32 banks.
// Returns nonzero, with a line on stdout, where one fails.
#pragma once
#include <cstdio>
#include <vector>

#include "../../sdrainer_amd/csrc/fft_f64.h"

template <class IM, int LOGN>
static int audit_image()
{
    using PL = fft64::Plan<LOGN>;
    constexpr int N = PL::N, SB = IM::SAMPLE_BYTES, PER_GRANULE = 16 / SB;
    int bad = 0;
    std::vector<int> owner(N, -1);
    for (int n = 0; n < N; n++) {
        const int a = IM::lds_byte(n);
        if (a < 0 || a >= SB * N || a % SB || owner[a / SB] >= 0) {
            std::printf("N=%d: sample %d -> byte %d (bad or taken)\n", N, n, a);
            return 1;
        }
        owner[a / SB] = n;
    }
    if (IM::ROWS_PER_WAVE * (PL::T / 64) != IM::ROWS || IM::ROWS * 1024 != SB * N) {
        std::printf("N=%d: %d waves x %d rows do not cover %d rows\n", N, PL::T / 64, IM::ROWS_PER_WAVE, IM::ROWS);
        return 1;
    }
    for (int r = 0; r < IM::ROWS; r++) {
        std::vector<int> seen(64, 0);
        for (int p = 0; p < 64; p++) {
            const int g = IM::granule(p, r);
            if (g < 0 || g >= 64 || seen[g]++) {
                std::printf("N=%d row %d: lane %d fetches granule %d (bad or twice)\n", N, r, p, g);
                return 1;
            }
            for (int i = 0; i < PER_GRANULE; i++)
                if (IM::lds_byte(r * IM::ROW_SAMPLES + g * PER_GRANULE + i) != r * 1024 + p * 16 + SB * i)
                    bad++;
        }
    }
    constexpr int WORD = SB > 4 ? SB : 4;
    for (int m = 0; m < PL::R; m++) {
        const int slot_byte = IM::lds_byte(fft64::input_sample<LOGN>(0, m));
        for (int t0 = 0; t0 < PL::T; t0 += 32) {
            int word_of_bank[32];
            unsigned banks = 0;
            for (int k = 0; k < 32; k++)
                word_of_bank[k] = -1;
            for (int t = t0; t < t0 + 32; t++) {
                const int a = IM::lds_byte(fft64::input_sample<LOGN>(t, 0)) ^ slot_byte;
                if (a != IM::lds_byte(fft64::input_sample<LOGN>(t, m)))
                    bad++;
                const int w = a / WORD, bank = w % 32;
                if (word_of_bank[bank] >= 0 && word_of_bank[bank] != w) {  // (another word of the same bank: one more cycle)
                    std::printf("N=%d slot %d threads %d..: bank conflict (bank %d)\n", N, m, t0, bank);
                    return 1;
                }
                word_of_bank[bank] = w;
                banks |= 1u << bank;
            }
            if (SB >= 4 && banks != 0xffffffffu) {
                std::printf("N=%d slot %d threads %d..: bank conflict (mask %08x)\n", N, m, t0, banks);
                return 1;
            }
        }
    }
    if (bad)
        std::printf("N=%d: %d address mismatches\n", N, bad);
    return bad != 0;
}

// every size the one-frame kernels are instantiated for
template <template <int> class IMAGE>
static int audit_images()
{
    return audit_image<IMAGE<9>, 9>() | audit_image<IMAGE<10>, 10>() | audit_image<IMAGE<11>, 11>() | audit_image<IMAGE<12>, 12>() |
           audit_image<IMAGE<13>, 13>() | audit_image<IMAGE<14>, 14>();
}
