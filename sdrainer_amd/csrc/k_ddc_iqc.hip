// k_ddc_iqc.hip — the down-converter's kernel over the corrected input traits (iq_correct.h): k_ddc<InCorrected<InF32>>,
// <InCorrected<InSc16>> and <InCorrected<InIq8>>, launched only while an IQ correction is set (capi_ddc.hip).  The kernel
// body and the arithmetic's contract are k_ddc.h; k_ddc.hip and k_ddc_real.hip keep exactly the kernels they hold.
#include "k_ddc.h"

#include "front_input.h"
#include "iq_correct.h"

namespace sdr {

hipError_t launch_ddc_iqc(const DdcLaunch &l, const sdr_iq_correction &c, hipStream_t stream)
{
    return with_complex_input(l.fmt, [&](auto in) { return launch_ddc_as(corrected(in, c), l, stream); });  // (no real format)
}

}  // namespace sdr
