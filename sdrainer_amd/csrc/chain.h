// chain.h — what an sdr_chain (capi_chain.hip, include/sdrainer_hip.h "receive chain") reads of the objects it borrows.  Each
// accessor is defined beside its object's struct (capi_nb.hip, capi_ddc.hip, capi_chan.hip, capi_fine.hip, capi_bank.hip) and
// reads only: no public behaviour of those files changes, and a process that never creates a chain never calls one.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sdrainer_hip.h"

namespace sdr {

// an object's configuration and the stream its process calls run on
const sdr_nb_config &nb_config(const sdr_nb *nb);
const sdr_ddc_config &ddc_config(const sdr_ddc *ddc);
const sdr_chan_config &chan_config(const sdr_chan *chan);
const sdr_fine_config &fine_config(const sdr_fine *fine);
hipStream_t nb_stream(const sdr_nb *nb);
hipStream_t ddc_stream(const sdr_ddc *ddc);
hipStream_t chan_stream(const sdr_chan *chan);
hipStream_t fine_stream(const sdr_fine *fine);

struct ChainBankView {
    int n_bands, block_size, hop, max_batch_frames, device_id;
    hipStream_t stream;   // the caller's stream: where the FFT reads the input (sdr_set_stream)
    bool graph_captured;  // sdr_graph_capture without a release
    bool input_staged;    // sdr_push_* input, or the history a staged batch left, on any band
    bool defer_listen;    // sdr_defer_listen on, or a batch waiting for its listen half
};
ChainBankView chain_bank_view(const sdr_bank *bank);

}  // namespace sdr
