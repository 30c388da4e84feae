// ddc_input_real.h — the input traits of the real formats (include/sdrainer_hip.h SDR_DDC_REAL), shared by the two units
// that convert a wide stream: k_ddc_real.hip (the down-converter) and k_chan.hip (the channelizer).  A real sample v is the
// complex sample (v, +0.0f); a value's float32 is what the complex format of the same sample type makes of that word
// (sc16.h, iq8.h).  kWide: samples per 16-byte load (k_ddc.h ddc_mix_wide).
#pragma once
#include "iq8.h"
#include "sc16.h"

namespace sdr {

struct InRealF32 {
    using word = float;
    static constexpr int kWide = 4;  // samples per 16-byte load (k_ddc.h ddc_mix_wide)
    __device__ __forceinline__ float re(word w) const { return w; }
    __device__ __forceinline__ float im(word) const { return 0.f; }
};

struct InRealS16 {
    using word = uint16_t;
    static constexpr int kWide = 8;  // samples per 16-byte load (k_ddc.h ddc_mix_wide)
    __device__ __forceinline__ float re(word w) const { return sc16::re_of(w); }
    __device__ __forceinline__ float im(word) const { return 0.f; }
};

// rs8 and ru8: which of the two is the trait's state, as InIq8 has it
struct InReal8 {
    using word = uint8_t;
    static constexpr int kWide = 16;  // samples per 16-byte load (k_ddc.h ddc_mix_wide)
    iq8::Format fmt;
    __device__ __forceinline__ float re(word w) const { return iq8::re_of(w, fmt); }
    __device__ __forceinline__ float im(word) const { return 0.f; }
};

}  // namespace sdr
