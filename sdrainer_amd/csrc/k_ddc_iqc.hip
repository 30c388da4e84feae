// k_ddc_iqc.hip — the down-converter's kernel over the corrected input traits (iq_correct.h): k_ddc<InCorrected<InF32>>,
// <InCorrected<InSc16>> and <InCorrected<InIq8>>, launched only while an IQ correction is set (capi_ddc.hip).  The kernel
// body and the arithmetic's contract are k_ddc.h; k_ddc.hip and k_ddc_real.hip keep exactly the kernels they hold.
#include "k_ddc.h"

#include "fft_input.h"
#include "iq_correct.h"

namespace sdr {

hipError_t launch_ddc_iqc(const DdcLaunch &l, const sdr_iq_correction &c, hipStream_t stream)
{
    switch (l.fmt) {
    case SDR_DDC_F32: return launch_ddc_as(corrected(InF32{}, c), l, stream);
    case SDR_DDC_SC16: return launch_ddc_as(corrected(InSc16{}, c), l, stream);
    case SDR_DDC_CS8: return launch_ddc_as(corrected(InIq8{iq8::format_of(false)}, c), l, stream);
    case SDR_DDC_CU8: return launch_ddc_as(corrected(InIq8{iq8::format_of(true)}, c), l, stream);
    }
    return hipErrorInvalidValue;  // (a real format has no correction)
}

}  // namespace sdr
