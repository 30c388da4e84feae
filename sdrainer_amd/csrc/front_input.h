// front_input.h — the input trait of a front-end format (include/sdrainer_hip.h SDR_DDC_*), format by format: the one table
// for the five units that launch k_ddc or k_chan per format.  f(trait) for a complex / a real format; hipErrorInvalidValue for
// a format of the other kind or none.  Two tables, so that a unit instantiates the kernels of one kind only.  cs8 / cu8 and
// rs8 / ru8 share a trait each: which of the two is the trait's state.
#pragma once
#include "ddc_input_real.h"
#include "fft_input.h"
#include "host/ddc_format.h"

namespace sdr {

template <class F>
hipError_t with_complex_input(int fmt, F &&f)
{
    switch (fmt) {
    case SDR_DDC_F32: return f(InF32{});
    case SDR_DDC_SC16: return f(InSc16{});
    case SDR_DDC_CS8:
    case SDR_DDC_CU8: return f(InIq8{iq8::format_of(fmt == SDR_DDC_CU8)});
    }
    return hipErrorInvalidValue;
}

template <class F>
hipError_t with_real_input(int fmt, F &&f)
{
    switch (fmt) {
    case SDR_DDC_RF32: return f(InRealF32{});
    case SDR_DDC_RS16: return f(InRealS16{});
    case SDR_DDC_RS8:
    case SDR_DDC_RU8: return f(InReal8{iq8::format_of(ddc_complex_base(fmt) == SDR_DDC_CU8)});
    }
    return hipErrorInvalidValue;
}

}  // namespace sdr
