// ddc.h — the digital down-converter in front of a bank (include/sdrainer_hip.h "down-converter"):
// what k_ddc.hip's launchers take, and the tile shape, which is plain constexpr arithmetic shared by host and kernel.
//
// One workgroup computes kDdcTileOutputs consecutive outputs of one band, in chunks of `chunk` outputs: a chunk's input
// span of (chunk - 1) * D + T samples is converted and mixed once and kept in LDS as (re, im) pairs, stored by polyphase -
// element i of the span in row i mod D, column i div D of a [D][width] image - so that for a fixed tap the lanes, which hold
// consecutive outputs, read one row at consecutive columns (conflict-free for any D; in sample order a power-of-two D
// would put every lane on one bank).  `width` is odd: consecutive samples, which the mixing lanes store, go to
// consecutive rows, width pairs apart.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/sdrainer_hip.h"

namespace sdr {

constexpr int kDdcNco = SDR_DDC_NCO_SIZE;             // L: entries of the NCO table
constexpr int kDdcTileOutputs = SDR_DDC_TILE_OUTPUTS;  // outputs of one band per workgroup
constexpr int kDdcMaxThreads = 256;
constexpr int kDdcOutputsPerThread = kDdcTileOutputs / kDdcMaxThreads;  // a lane's outputs of a chunk: lane, lane + threads
constexpr int kDdcMaxLdsBytes = 160 * 1024;                              // the whole LDS of a CU
constexpr int kDdcMaxBands = 64, kDdcMaxDecimation = 256, kDdcMaxTaps = 4096;
static_assert(kDdcTileOutputs == kDdcMaxThreads * kDdcOutputsPerThread, "a chunk is at most two outputs per lane");

// the image's row width in (re, im) pairs for a chunk of c outputs
constexpr int ddc_width(int c, int d, int t) { return (((c - 1) * d + t + d - 1) / d) | 1; }

struct DdcShape {
    int chunk;    // outputs per chunk: <= kDdcTileOutputs, a multiple of 64 where 64 fit
    int width;    // ddc_width(chunk, D, T)
    int threads;  // workgroup size: a multiple of 64, chunk <= kDdcOutputsPerThread * threads
    unsigned lds_bytes;
};

// The largest chunk whose image fits kDdcMaxLdsBytes (D = 256, T = 4096: 64 outputs); whole waves where 64 outputs fit.
constexpr DdcShape ddc_shape(int d, int t)
{
    int c = kDdcTileOutputs;
    while (c > 1 && (long long)d * ddc_width(c, d, t) * 8 > kDdcMaxLdsBytes)
        c--;
    if (c >= 64)
        c -= c % 64;
    int threads = (c + 63) / 64 * 64;
    if (threads > kDdcMaxThreads)
        threads = kDdcMaxThreads;
    return DdcShape{c, ddc_width(c, d, t), threads, (unsigned)(d * ddc_width(c, d, t) * 8)};
}
static_assert(ddc_shape(kDdcMaxDecimation, kDdcMaxTaps).lds_bytes <= (unsigned)kDdcMaxLdsBytes, "the largest geometry fits");
static_assert(ddc_shape(1, kDdcMaxTaps).lds_bytes <= (unsigned)kDdcMaxLdsBytes && ddc_shape(1, 1).chunk == kDdcTileOutputs, "");

// the bands' tuning steps travel as a launch argument: a retune between two calls never touches memory a kernel reads
struct DdcSteps {
    int16_t step[kDdcMaxBands];
};

struct DdcLaunch {
    int fmt;             // SDR_DDC_F32 .. SDR_DDC_CU8
    const void *in;      // this call's n_in raw samples
    const void *carry;   // the n_taps - 1 raw samples in front of them (sample first - (T - 1) + i at [i])
    const float2 *nco;   // [kDdcNco] (cos, sin)
    const float *taps;   // [n_taps]
    float *out;          // band b's outputs from float pair b * out_stride on
    size_t out_stride;
    long long first;     // K: the stream index of in[0], a multiple of D
    long long origin;    // samples below this index are zero (the DDC's first sample)
    int n_in, n_bands, decimation, n_taps;
    DdcSteps steps;
};

hipError_t launch_ddc(const DdcLaunch &l, hipStream_t stream);
// k_ddc_iqc.hip: the same kernel over the corrected traits (iq_correct.h), for the four complex formats only
hipError_t launch_ddc_iqc(const DdcLaunch &l, const sdr_iq_correction &c, hipStream_t stream);
// carry_out = the last n_taps - 1 samples of (carry_in, in[0 .. n_in)); carry_out != carry_in
hipError_t launch_ddc_carry(int fmt, const void *carry_in, const void *in, int n_in, int n_taps, void *carry_out, hipStream_t stream);

}  // namespace sdr
