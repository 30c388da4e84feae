// k_chan.hip — the channelizer's kernel over every input format of the down-converter: the four complex traits of
// fft_input.h and the three real ones of ddc_input_real.h (cs8 / cu8 and rs8 / ru8 share a trait each).  The kernel body and
// the arithmetic's contract are k_chan.h.
#include "k_chan.h"

#include "ddc_input_real.h"
#include "fft_input.h"
#include "host/ddc_format.h"

namespace sdr {

hipError_t launch_chan(const ChanLaunch &l, hipStream_t stream)
{
    switch (l.fmt) {
    case SDR_DDC_F32: return launch_chan_as(InF32{}, l, stream);
    case SDR_DDC_SC16: return launch_chan_as(InSc16{}, l, stream);
    case SDR_DDC_CS8:
    case SDR_DDC_CU8: return launch_chan_as(InIq8{iq8::format_of(l.fmt == SDR_DDC_CU8)}, l, stream);
    case SDR_DDC_RF32: return launch_chan_as(InRealF32{}, l, stream);
    case SDR_DDC_RS16: return launch_chan_as(InRealS16{}, l, stream);
    case SDR_DDC_RS8:
    case SDR_DDC_RU8: return launch_chan_as(InReal8{iq8::format_of(ddc_complex_base(l.fmt) == SDR_DDC_CU8)}, l, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace sdr
