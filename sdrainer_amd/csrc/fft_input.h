// fft_input.h — what an FFT kernel needs from an input format, stated once per format: the word a sample is read as (its
// size is the bytes per sample), the BatchCursor field that carries a replayed graph's pointer, the staging image of the
// one-frame kernels (fft_f64.h "Input staging") and the float32 value of a word's two components.  k_fft_psd.h's one-frame
// body and k_fft_2p_a.h's input loop are written over these, and the kernel templates take them as template arguments; the conversions themselves are sc16.h's and iq8.h's.
#pragma once
#include "iq8.h"
#include "sc16.h"
#include "sdr_device.h"

namespace sdr {

struct InF32 {
    using word = float2;
    template <int LOGN>
    using Image = fft64::InImageF32<LOGN>;
    static __device__ __forceinline__ const void *replayed(const BatchCursor &c) { return c.iq; }
    __device__ __forceinline__ float re(word w) const { return w.x; }
    __device__ __forceinline__ float im(word w) const { return w.y; }
};

struct InSc16 {
    using word = uint32_t;
    template <int LOGN>
    using Image = sc16::Image<LOGN>;
    static __device__ __forceinline__ const void *replayed(const BatchCursor &c) { return c.iq_sc16; }
    __device__ __forceinline__ float re(word w) const { return sc16::re_of(w); }
    __device__ __forceinline__ float im(word w) const { return sc16::im_of(w); }
};

// cs8 and cu8: which of the two is the trait's state (a launch argument of the one-frame kernels, a constant in phase A)
struct InIq8 {
    using word = uint16_t;
    template <int LOGN>
    using Image = iq8::Image<LOGN>;
    iq8::Format fmt;
    static __device__ __forceinline__ const void *replayed(const BatchCursor &c) { return c.iq8; }
    __device__ __forceinline__ float re(word w) const { return iq8::re_of(w, fmt); }
    __device__ __forceinline__ float im(word w) const { return iq8::im_of(w, fmt); }
};

template <InFormat FMT>
__device__ __forceinline__ constexpr auto input_of()
{
    if constexpr (FMT == InFormat::F32)
        return InF32{};
    else if constexpr (FMT == InFormat::SC16)
        return InSc16{};
    else
        return InIq8{iq8::format_of(FMT == InFormat::CU8)};
}

// the frames a launch reads: the launch argument, or in graph replay the batch's pointer in device memory
template <class IN>
__device__ __forceinline__ const typename IN::word *input_frames(const void *iq_arg, const BatchCursor *cur)
{
    return static_cast<const typename IN::word *>(cur ? IN::replayed(*cur) : iq_arg);
}

}  // namespace sdr
