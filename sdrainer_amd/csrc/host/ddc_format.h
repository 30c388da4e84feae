// host/ddc_format.h — the down-converter's input formats (include/sdrainer_hip.h SDR_DDC_*) as plain constexpr arithmetic:
// which ints are formats, which are real, the complex format of the same sample type and the bytes of one sample.  No HIP
// include: capi_ddc.hip and the launchers use it, tests/host/test_ddc_format.cpp walks it on the host.
#pragma once
#include "../../../include/sdrainer_hip.h"

namespace sdr {

// a format is a sample type (SDR_DDC_F32 .. SDR_DDC_CU8) with or without SDR_DDC_REAL, and nothing else
constexpr bool ddc_format_valid(int fmt) { return (fmt & ~(SDR_DDC_REAL | SDR_DDC_CU8)) == 0; }
constexpr bool ddc_is_real(int fmt) { return (fmt & SDR_DDC_REAL) != 0; }
// the complex format whose conversion gives a raw value its float32 value
constexpr int ddc_complex_base(int fmt) { return fmt & SDR_DDC_CU8; }
// bytes of one raw sample: a complex sample is two values, a real one is one
constexpr int ddc_sample_bytes(int fmt)
{
    const int base = ddc_complex_base(fmt);
    const int value = base == SDR_DDC_F32 ? 4 : base == SDR_DDC_SC16 ? 2 : 1;
    return ddc_is_real(fmt) ? value : 2 * value;
}

static_assert(SDR_DDC_CU8 == 3 && SDR_DDC_REAL == 16, "the sample type is the low two bits, the real flag stands clear of them");
static_assert(SDR_DDC_RF32 == (SDR_DDC_REAL | SDR_DDC_F32) && SDR_DDC_RS16 == (SDR_DDC_REAL | SDR_DDC_SC16), "");
static_assert(SDR_DDC_RS8 == (SDR_DDC_REAL | SDR_DDC_CS8) && SDR_DDC_RU8 == (SDR_DDC_REAL | SDR_DDC_CU8), "");

}  // namespace sdr
