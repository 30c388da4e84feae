// iq_sums_dev.h — the raw-stream sums of one down-converter or channelizer (include/sdrainer_hip.h "IQ correction"): what
// capi_ddc.hip and capi_chan.hip hold and call, implemented by k_iq_sums.hip.  The five sums live in a device record in
// units u (host/iq_sums.h); n and skipped are host counters.  Everything is ordered by the object's one stream.
#pragma once
#include <hip/hip_runtime.h>

#include "host/iq_sums.h"

namespace sdr {

// one workgroup of k_iq_sums sums this many 16-byte groups: 16 per lane, so that an 8-bit lane's int32 accumulators hold
// at most 128 squares below 2^16
constexpr int kIqSumsThreads = 256, kIqSumsGroupsPerLane = 16;
constexpr int kIqSumsBlockGroups = kIqSumsThreads * kIqSumsGroupsPerLane;
constexpr int kIqSumsValues = 5;  // sum_i, sum_q, sum_ii, sum_qq, sum_iq

// workgroups for n samples of a format: every whole group and, where the samples do not fill the last one, the ragged end
constexpr long long iq_sums_blocks(int fmt, long long n)
{
    const long long per = 16 / ddc_sample_bytes(fmt), groups = (n + per - 1) / per;
    return groups > 0 ? (groups + kIqSumsBlockGroups - 1) / kIqSumsBlockGroups : 1;
}

struct IqSums {
    bool on = false;
    IqSumsCount count;            // n and skipped since the last read
    long long *d_rec = nullptr;   // [kIqSumsValues], units u
    long long *d_part = nullptr;  // [iq_sums_blocks(max_in_samples)][kIqSumsValues]: the workgroups' partial sums of one call
};

// on: allocates at the first use (for calls of up to max_in_samples); on or off, the sums are cleared
hipError_t iq_sums_enable(IqSums &s, int fmt, int max_in_samples, bool on, hipStream_t stream);
// the sums of this call's n_in raw samples, added to the record behind whatever the stream holds (or counted as skipped)
hipError_t iq_sums_add(IqSums &s, int fmt, const void *in, int n_in, hipStream_t stream);
// waits for the stream, fills *out and clears
hipError_t iq_sums_read(IqSums &s, sdr_iq_sums *out, hipStream_t stream);
void iq_sums_free(IqSums &s);

}  // namespace sdr
