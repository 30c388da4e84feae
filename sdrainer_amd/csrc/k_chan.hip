// k_chan.hip — the channelizer's kernel over every input format of the down-converter: the four complex traits of
// fft_input.h and the three real ones of ddc_input_real.h (cs8 / cu8 and rs8 / ru8 share a trait each).  The kernel body and
// the arithmetic's contract are k_chan.h.
#include "k_chan.h"

#include "front_input.h"

namespace sdr {

hipError_t launch_chan(const ChanLaunch &l, hipStream_t stream)
{
    const auto launch = [&](auto in) { return launch_chan_as(in, l, stream); };
    return !ddc_is_real(l.fmt) ? with_complex_input(l.fmt, launch) : with_real_input(l.fmt, launch);
}

}  // namespace sdr
