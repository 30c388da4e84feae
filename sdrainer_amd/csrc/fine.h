// fine.h — the fine converter behind a channelizer or a first DDC (include/sdrainer_hip.h "fine converter", DESIGN.md section
// 1): what k_fine.hip's launchers take.  The tile, the chunks and the polyphase LDS image are the down-converter's (ddc.h
// ddc_shape), which this object shares by inclusion; what differs is that every band reads a stream of its own.
#pragma once
#include "ddc.h"

namespace sdr {

constexpr int kFineMaxBands = kDdcMaxBands, kFineMaxInputs = 256;
static_assert(kFineMaxInputs - 1 <= 255, "an input index travels as one byte");

// the bands' steps and the input each band reads travel as a launch argument (as DdcSteps does): a retune or a re-pointing
// between two calls never touches memory a kernel reads
struct FineMap {
    int16_t step[kFineMaxBands];
    uint8_t input[kFineMaxBands];
};

struct FineLaunch {
    const float2 *in;     // input i's n_in samples from in + i * in_stride on
    size_t in_stride;
    const float2 *carry;  // [n_inputs][n_taps - 1]: the samples in front of them, per input (sample first - (T - 1) + j at [j])
    const float2 *nco;    // [kDdcNco] (cos, sin)
    const float *taps;    // [n_taps]
    float *out;           // band b's outputs from float pair b * out_stride on
    size_t out_stride;
    long long first;      // K: the index of every input's in[0], a multiple of D
    long long origin;     // samples below this index are zero
    int n_in, n_bands, n_inputs, decimation, n_taps;
    FineMap map;
};

hipError_t launch_fine(const FineLaunch &l, hipStream_t stream);
// carry_out[i] = the last n_taps - 1 samples of (carry_in[i], input i's in[0 .. n_in)) for every input; carry_out != carry_in
hipError_t launch_fine_carry(const float2 *carry_in, const float2 *in, size_t in_stride, int n_in, int n_inputs, int n_taps,
                             float2 *carry_out, hipStream_t stream);

}  // namespace sdr
