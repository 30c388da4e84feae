// iq_correct.h — the IQ correction as an input trait (include/sdrainer_hip.h "IQ correction"): InCorrected<IN> wraps a complex
// input trait of fft_input.h, reads the same word and gives the corrected float32 (re, im).  With (re0, im0) the base
// trait's values, each line one float32 operation rounded on its own (the library is built with -ffp-contract=off):
//     re1 = re0 - dc_re          im1 = im0 - dc_im
//     re  = re1                  im  = (gain_im * im1) + (cross * re1)
// k_ddc.h and k_chan.h read a sample only through fmt.re and fmt.im, and write the zero samples below the first sample
// without the trait: those stay (+0, +0).  The instances are k_ddc_iqc.hip's and k_chan_iqc.hip's.
#pragma once
#include <type_traits>

#include "../../include/sdrainer_hip.h"
#include "sdr_device.h"

namespace sdr {

// a base trait that asks for wide loads (kWide, k_ddc.h) keeps asking for them
template <class IN, class = void>
struct InCorrectedWide {};
template <class IN>
struct InCorrectedWide<IN, std::void_t<decltype(IN::kWide)>> {
    static constexpr int kWide = IN::kWide;
};

template <class IN>
struct InCorrected : InCorrectedWide<IN> {
    using word = typename IN::word;
    IN base;
    sdr_iq_correction c;
    __device__ __forceinline__ float re(word w) const { return base.re(w) - c.dc_re; }
    __device__ __forceinline__ float im(word w) const
    {
        const float re1 = base.re(w) - c.dc_re;
        const float im1 = base.im(w) - c.dc_im;
        return (c.gain_im * im1) + (c.cross * re1);
    }
};

template <class IN>
inline InCorrected<IN> corrected(IN base, const sdr_iq_correction &c)
{
    InCorrected<IN> t{};
    t.base = base;
    t.c = c;
    return t;
}

}  // namespace sdr
