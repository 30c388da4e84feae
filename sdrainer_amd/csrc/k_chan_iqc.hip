// k_chan_iqc.hip — the channelizer's kernel over the corrected input traits (iq_correct.h): k_chan<InCorrected<InF32>>,
// <InCorrected<InSc16>> and <InCorrected<InIq8>>, launched only while an IQ correction is set (capi_chan.hip).  The kernel
// body and the arithmetic's contract are k_chan.h; k_chan.hip keeps exactly the kernels it holds.
#include "k_chan.h"

#include "front_input.h"
#include "iq_correct.h"

namespace sdr {

hipError_t launch_chan_iqc(const ChanLaunch &l, const sdr_iq_correction &c, hipStream_t stream)
{
    return with_complex_input(l.fmt, [&](auto in) { return launch_chan_as(corrected(in, c), l, stream); });  // (no real format)
}

}  // namespace sdr
