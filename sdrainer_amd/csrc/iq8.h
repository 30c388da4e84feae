// iq8.h — complex 8-bit input, two bytes per sample (I, then Q), read by the FFT kernels themselves (k_fft_psd_iq8.hip,
// k_fft_r32_iq8.hip, k_fft_2p_iq8.hip) and unpacked by k_unpack.hip for the staged host path.  Two formats:
//   cs8  int8_t   value = float32(x) / 128                              (HackRF class)
//   cu8  uint8_t  value = (float32(x) - 127.5) / 128 = (2 x - 255) / 256  (RTL-SDR class)
// Both are exact in float32 for all 256 inputs: nothing is rounded, so an 8-bit batch gives exactly the bits of the float32
// batch of those values.  One code path serves both: u = x ^ flip as an unsigned byte, value = u * (1/128) - c, with
// flip = 0x80, c = 1 for cs8 (x ^ 0x80 is x + 128) and flip = 0, c = 255/256 for cu8.  The FMA is explicit - the library is
// compiled with -ffp-contract=off - and exact: |2 u - 255| < 2^9.
//
// Everything here is SDR_HD and free of HIP intrinsics: tests/host/test_iq8_host.cpp compiles this very header on the CPU,
// checks both conversions for all 256 inputs against the exact rationals and audits the staging image.
#pragma once
#include <cstdint>

#include "fft_f64.h"

namespace iq8 {

// what a kernel is told about the format: the XOR mask of a 16-bit sample word (both bytes) and the constant c
struct Format {
    uint32_t flip;  // 0x8080 (cs8) or 0 (cu8)
    float c;        // 1 (cs8) or 255/256 (cu8)
};
SDR_HD constexpr Format format_of(bool cu8) { return cu8 ? Format{0u, 255.0f / 256.0f} : Format{0x8080u, 1.0f}; }

// u: the byte XORed with its half of Format::flip, 0 .. 255
SDR_HD inline float to_f32(uint32_t u, float c) { return __builtin_fmaf((float)u, 1.0f / 128.0f, -c); }

// one 16-bit word = one sample: I in the low byte, Q in the high byte
SDR_HD inline float re_of(uint32_t w, Format f) { return to_f32((w ^ f.flip) & 0xffu, f.c); }
SDR_HD inline float im_of(uint32_t w, Format f) { return to_f32(((w ^ f.flip) >> 8) & 0xffu, f.c); }

// ---------------------------------------------------------------------------------------------
// The staging image of k_fft_psd_narrow<InIq8, ..> (the float32 kernel's is fft_f64.h "Input staging", the sc16 kernel's sc16.h): the
// frame is copied global -> LDS by LDS-DMA, one contiguous 1 KB row of 512 samples per wave instruction, 16 bytes (a
// granule of eight samples) per lane, and read back in the pass-0 layout with one 16-bit LDS read per register slot.  Such
// a read is served in two groups of 32 lanes over 32 four-byte banks; two lanes that read the two halves of ONE dword do
// not conflict.  Pass 0's lane bits 0 and 1 are sample bits 0 and 1: lanes 2 j and 2 j + 1 share a dword, and lane bit 1 is
// dword-address bit 0.  Lane bits 2-4 are higher sample bits: sample bit 2 is dword bit 1 (inside the granule), sample
// bits 3-5 are granule-position bits 0-2 (dword bits 2-4) of a linear image; a lane bit that holds a sample bit above 5
// gets a position bit no other lane bit sits on, XORed with its sample bit.  The DMA writes lane l's granule at row base
// + 16 l, so the swizzle is applied through the SOURCE address.
//   sample n  ->  row r = n >> 9, granule g = (n >> 3) & 63, byte r*1024 + pos(g, r)*16 + (n & 7)*2
// Every source bit is a granule bit above 2 (N <= 16384: the highest lane-held sample bit is 8, granule bit 5), so the map
// is triangular and its own inverse is found downwards: pos, granule and lds_byte are fft64::InImage's (fft_f64.h "Input
// staging"), with eight samples per granule and the rule below in place of the other two images' pairing.
// ---------------------------------------------------------------------------------------------
// The rule: which bit each position bit is XORed with (fft64::InSwz).
template <int LOGN>
struct FirstFreeSwz {
    SDR_HD static constexpr fft64::InSwz make()
    {
        const fft64::Layout L0 = fft64::make_layout<LOGN>(0);
        fft64::InSwz z{0, {-1, -1, -1}};
        bool taken[3] = {false, false, false};
        int nbs[3] = {0, 0, 0};
        for (int k = 0; k < 3; k++) {
            nbs[k] = LOGN - 1 - L0.tbit[2 + k];  // sample-number bit behind lane bit 2+k
            if (nbs[k] >= 3 && nbs[k] <= 5)
                taken[nbs[k] - 3] = true;  // sits on a position bit of the linear image already
        }
        for (int k = 0; k < 3; k++) {
            if (nbs[k] <= 5)
                continue;  // (2: dword bit 1, inside the granule)
            int j = 0;
            while (j < 3 && taken[j])
                j++;
            if (j == 3)
                continue;  // (cannot happen: three lane bits, three position bits)
            taken[j] = true;
            z.src[j] = nbs[k] >= 9 ? 8 + (nbs[k] - 9) : nbs[k] - 3;
        }
        return z;
    }
};

template <int LOGN>
using Image = fft64::InImage<LOGN, 3, FirstFreeSwz<LOGN>>;
// the image's functions and row counts by the format's own names (the kernel and the host audits call either)
template <int LOGN>
SDR_HD inline int granule(int p, int r) { return Image<LOGN>::granule(p, r); }
template <int LOGN>
SDR_HD inline int lds_byte(int n) { return Image<LOGN>::lds_byte(n); }
template <int LOGN>
constexpr int kRows = Image<LOGN>::ROWS;
template <int LOGN>
constexpr int kRowsPerWave = Image<LOGN>::ROWS_PER_WAVE;

}  // namespace iq8
