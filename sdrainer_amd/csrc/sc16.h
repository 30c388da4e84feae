// sc16.h — complex int16 input ("sc16": int16 I, then int16 Q, little-endian), read by the FFT kernels themselves
// (k_fft_psd.h k_fft_psd_narrow<InSc16, ..>, k_fft_r32_sc16.hip) and unpacked by k_unpack.hip for the staged host path.
//
// A sample's value is float32(x) / 32767, correctly rounded: the reference's float32(int16(v)) / float32(math.MaxInt16)
// (kiwi/client.go:298-308), and what k_unpack.hip's be16_to_f32 computes with a division.  Everything after the
// conversion is the float32 path's, so an sc16 batch gives exactly the bits of the float32 batch of those values.
//
// Everything here is SDR_HD and free of HIP intrinsics: tests/host/test_sc16_host.cpp compiles this very header on the
// CPU, checks the conversion against a correctly rounded division for all 65 536 inputs and audits the staging image.
#pragma once
#include <cstdint>

#include "fft_f64.h"

namespace sc16 {

// x / 32767 rounded once.  A plain multiply by the rounded reciprocal is off by one unit in the last place for 1 536 of
// the 65 536 inputs; one FMA step on its residual fixes every one of them (exhaustively checked, see above).  The FMAs
// are explicit: the library is compiled with -ffp-contract=off, and nothing else here may fuse.
SDR_HD inline float to_f32(int16_t x)
{
    constexpr float kInv = 1.0f / 32767.0f;
    const float xf = (float)x;
    const float q0 = xf * kInv;
    const float r = __builtin_fmaf(-q0, 32767.0f, xf);  // exact: the residual of a faithful quotient
    return __builtin_fmaf(r, kInv, q0);
}

// one 32-bit word = one sample: I in the low half, Q in the high half (little-endian)
SDR_HD inline float re_of(uint32_t w) { return to_f32((int16_t)(uint16_t)(w & 0xffffu)); }
SDR_HD inline float im_of(uint32_t w) { return to_f32((int16_t)(uint16_t)(w >> 16)); }

// ---------------------------------------------------------------------------------------------
// The staging image of k_fft_psd_narrow<InSc16, ..> (the float32 kernel's is fft_f64.h "Input staging"): the frame is copied global ->
// LDS by LDS-DMA, one contiguous 1 KB row of 256 samples per wave instruction, 16 bytes (a granule of four samples) per
// lane, and read back in the pass-0 layout with one ds_read_b32 per register slot.  A ds_read_b32 is served in two
// groups of 32 lanes over 32 four-byte banks: the 32 lanes' words must differ mod 32, i.e. in word-address bits 0-4.
// Pass 0's lane bits 0 and 1 are sample bits 0 and 1 (word bits 0-1 of a linear image); lane bits 2-4 are higher sample
// bits in general, so granule-position bit k (word bit 2 + k) is XORed with the sample bit behind lane bit 2 + k
// (fft64::PairedSwz).  The DMA writes lane l's granule at row base + 16 l, so the swizzle is applied through the SOURCE
// address; pos, granule and lds_byte are fft64::InImage's (fft_f64.h "Input staging"), with four samples per granule.
//   sample n  ->  row r = n >> 8, granule g = (n >> 2) & 63, byte r*1024 + pos(g, r)*16 + (n & 3)*4
// ---------------------------------------------------------------------------------------------
template <int LOGN>
using Image = fft64::InImage<LOGN, 2>;
// the image's functions by the format's own names (the kernel and the host audits call either)
template <int LOGN>
SDR_HD inline int granule(int p, int r) { return Image<LOGN>::granule(p, r); }
template <int LOGN>
SDR_HD inline int lds_byte(int n) { return Image<LOGN>::lds_byte(n); }

}  // namespace sc16
