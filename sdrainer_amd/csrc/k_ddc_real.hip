// k_ddc_real.hip — the down-converter's kernel over the real input formats (include/sdrainer_hip.h SDR_DDC_REAL): one value
// per sample, as a direct-sampling receiver's ADC delivers it.  A real sample v is the complex sample (v, +0.0f) through
// k_ddc.h's arithmetic, bit for bit: the traits (ddc_input_real.h) give im = +0.0f and nothing else differs - the same two mix formulas
// (no product is dropped: 0 * s carries s's sign into the sum, and a NaN or Inf sample reaches both outputs), the same
// filter, the same image.  A value's float32 is what the complex format of the same sample type makes of that word
// (sc16.h, iq8.h).  The traits ask for 16-byte loads of 4, 8 or 16 samples (kWide, k_ddc.h ddc_mix_wide): with one word
// per lane rs16 measured 1 % behind sc16 at D = 8 and only 3 % ahead at D = 64 and 256, with the wide loads 18 % and 31 %
// ahead at D = 64 and 256 and 9 % behind at D = 8 (profiles/ddc_real_rate.json).
#include "k_ddc.h"

#include "front_input.h"

namespace sdr {

// (the traits InRealF32, InRealS16 and InReal8 are ddc_input_real.h's: the channelizer converts with them too)

hipError_t launch_ddc_real(const DdcLaunch &l, hipStream_t stream)
{
    return with_real_input(l.fmt, [&](auto in) { return launch_ddc_as(in, l, stream); });
}

hipError_t launch_ddc_carry_byte(const void *carry_in, const void *in, int n_in, int keep, void *carry_out, hipStream_t stream)
{
    return launch_carry_as<InReal8::word>(carry_in, in, n_in, keep, carry_out, stream);
}

}  // namespace sdr
