// k_chan_iqc.hip — the channelizer's kernel over the corrected input traits (iq_correct.h): k_chan<InCorrected<InF32>>,
// <InCorrected<InSc16>> and <InCorrected<InIq8>>, launched only while an IQ correction is set (capi_chan.hip).  The kernel
// body and the arithmetic's contract are k_chan.h; k_chan.hip keeps exactly the kernels it holds.
#include "k_chan.h"

#include "fft_input.h"
#include "iq_correct.h"

namespace sdr {

hipError_t launch_chan_iqc(const ChanLaunch &l, const sdr_iq_correction &c, hipStream_t stream)
{
    switch (l.fmt) {
    case SDR_DDC_F32: return launch_chan_as(corrected(InF32{}, c), l, stream);
    case SDR_DDC_SC16: return launch_chan_as(corrected(InSc16{}, c), l, stream);
    case SDR_DDC_CS8:
    case SDR_DDC_CU8: return launch_chan_as(corrected(InIq8{iq8::format_of(l.fmt == SDR_DDC_CU8)}, c), l, stream);
    }
    return hipErrorInvalidValue;  // (a real format has no correction)
}

}  // namespace sdr
