// chan.h — the polyphase channelizer in front of a bank (include/sdrainer_hip.h "channelizer"): what
// k_chan.hip's launcher takes, and the tile shape, which is plain constexpr arithmetic shared by host and kernel.
//
// One workgroup of kChanThreads lanes computes a tile of R consecutive output times of all M channels, R * M = kChanTileItems
// for every M, so a lane always has kChanTileItems / kChanThreads branch sums and half as many butterflies per FFT stage.
// Its LDS holds the tile's input span of (R - 1) * D + T samples as (re, im) pairs in sample order, and behind it the
// [R][M + 1] image the FFT runs in: the odd pitch lets the transposed store read one channel's R values from R banks.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/sdrainer_hip.h"

namespace sdr {

constexpr int kChanThreads = 256;
constexpr int kChanLogItems = 12, kChanTileItems = 1 << kChanLogItems;  // R * M
constexpr int kChanItemsPerThread = kChanTileItems / kChanThreads;      // a lane's branch sums
constexpr int kChanMaxLdsBytes = 160 * 1024;                             // the whole LDS of a CU
constexpr int kChanMaxChannels = 256, kChanMaxTaps = 4096, kChanMaxPhases = 64;

// log2 M for a legal geometry, -1 otherwise: M a power of two in 2 .. 256, D one of M, M/2, M/4 and at least 1,
// T = P * M with 1 <= P <= 64 and T <= 4096
constexpr int chan_log_m(int m, int d, int t)
{
    if (m < 2 || m > kChanMaxChannels || (m & (m - 1)) != 0)
        return -1;
    if (d < 1 || (d != m && d * 2 != m && d * 4 != m))
        return -1;
    if (t < m || t > kChanMaxTaps || t % m != 0 || t / m > kChanMaxPhases)
        return -1;
    int l = 0;
    while ((1 << l) < m)
        l++;
    return l;
}

struct ChanShape {
    int log_m;
    int tile;       // R: output times per workgroup
    int pitch;      // the image's row pitch in (re, im) pairs
    int span;       // (R - 1) * D + T: pairs of the span, which begins the LDS; the image follows it
    unsigned lds_bytes;
};

constexpr ChanShape chan_shape(int m, int d, int t)
{
    const int l = chan_log_m(m, d, t);
    if (l < 0)
        return ChanShape{-1, 0, 0, 0, 0};
    const int r = kChanTileItems >> l, span = (r - 1) * d + t;
    return ChanShape{l, r, m + 1, span, (unsigned)((span + r * (m + 1)) * 8)};
}
static_assert(chan_shape(256, 64, 4096).tile == 16 && chan_shape(2, 1, 2).tile == 2048, "");
static_assert(chan_shape(64, 64, 4096).lds_bytes <= (unsigned)kChanMaxLdsBytes && chan_shape(2, 2, 128).lds_bytes <= (unsigned)kChanMaxLdsBytes, "");
static_assert(chan_shape(256, 256, 4096).lds_bytes <= (unsigned)kChanMaxLdsBytes, "the largest geometries fit");

struct ChanLaunch {
    int fmt;              // SDR_DDC_F32 .. SDR_DDC_RU8
    const void *in;       // this call's n_in raw samples
    const void *carry;    // the n_taps - 1 raw samples in front of them (sample first - (T - 1) + i at [i])
    const float2 *nco;    // [SDR_DDC_NCO_SIZE] (cos, sin): the FFT's twiddles
    const float *taps;    // [n_taps]
    const int *channels;  // [n_out]: the channel of output stream i
    float *out;           // stream i's outputs from float pair i * out_stride on
    size_t out_stride;
    long long first;      // K: the stream index of in[0], a multiple of D
    long long origin;     // samples below this index are zero (the channelizer's first sample)
    int n_in, n_out, n_channels, decimation, n_taps;
};

hipError_t launch_chan(const ChanLaunch &l, hipStream_t stream);
// k_chan_iqc.hip: the same kernel over the corrected traits (iq_correct.h), for the four complex formats only
hipError_t launch_chan_iqc(const ChanLaunch &l, const sdr_iq_correction &c, hipStream_t stream);

}  // namespace sdr
