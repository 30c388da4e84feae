// k_ddc.hip — the down-converter's kernel over the four complex input formats (fft_input.h), and the launchers of every
// format.  The kernel bodies and the arithmetic's contract are k_ddc.h; the real formats' instances are k_ddc_real.hip.
#include "k_ddc.h"

#include "front_input.h"

namespace sdr {

hipError_t launch_ddc(const DdcLaunch &l, hipStream_t stream)
{
    const auto launch = [&](auto in) { return launch_ddc_as(in, l, stream); };
    return ddc_is_real(l.fmt) ? launch_ddc_real(l, stream) : with_complex_input(l.fmt, launch);
}

// the carry moves raw words: the kernel is chosen by the sample's size alone
hipError_t launch_ddc_carry(int fmt, const void *carry_in, const void *in, int n_in, int n_taps, void *carry_out, hipStream_t stream)
{
    const int keep = n_taps - 1;
    if (keep <= 0)
        return hipSuccess;
    if (!ddc_format_valid(fmt))
        return hipErrorInvalidValue;
    switch (ddc_sample_bytes(fmt)) {
    case 8: return launch_carry_as<InF32::word>(carry_in, in, n_in, keep, carry_out, stream);
    case 4: return launch_carry_as<InSc16::word>(carry_in, in, n_in, keep, carry_out, stream);
    case 2: return launch_carry_as<InIq8::word>(carry_in, in, n_in, keep, carry_out, stream);
    case 1: return launch_ddc_carry_byte(carry_in, in, n_in, keep, carry_out, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace sdr
