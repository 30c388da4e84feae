// k_chan.h — the polyphase channelizer's kernel body (chan.h, DESIGN.md section 1 "The channelizer"): one wide stream becomes
// M equally spaced float32 bands with T multiply-adds and one M-point FFT per output time.  The arithmetic is a contract,
// bit for bit (include/sdrainer_hip.h "channelizer"; tests/chan_ref.py is its NumPy restatement).  Per output time n:
//     branch sums   u[r] = sum over p = 0 .. P-1, in this order, of h[r + p M] * x[n D - r - p M]   (acc starts at +0)
//     rotation      v[r] = u[(r + n D) mod M]
//     FFT           a[i] = v[bitrev(i)]; radix-2 decimation in time with w = (COS, SIN)[q L / len], every twiddle multiplied
// every product and every sum rounded on its own (the library is built with -ffp-contract=off), subnormals kept.
//
// A workgroup takes a tile of R output times (chan.h) in four steps with a barrier between them:
//   1. all lanes convert the tile's input span to (re, im) pairs in LDS, 16 bytes of raw input per load where a group lies
//      inside the call's input, sample by sample across the carry, the origin and the span's ends;
//   2. lane <-> branch r is fixed (r = tid mod M): a lane walks its P taps once and accumulates its kChanItemsPerThread
//      output times side by side; lanes of one output time read consecutive (descending) span pairs.  A sum is written to
//      the image at the rotated and bit-reversed place, so the FFT runs in place and ends in channel order;
//   3. log2 M stages of R M / 2 butterflies dealt over the lanes, twiddles from the NCO table;
//   4. the selected channels are stored, each as R consecutive pairs.
// A last tile with fewer than R output times computes the rows behind them from whatever the LDS holds and stores none of it.
#pragma once
#include "chan.h"
#include "sdr_device.h"

namespace sdr {

template <class IN>
__device__ __forceinline__ void chan_convert(IN fmt, const typename IN::word *__restrict__ in, const typename IN::word *__restrict__ carry,
                                             float2 *__restrict__ span, long long first, long long origin, long long rel0, int len,
                                             int n_in, int T, int tid)
{
    using W = typename IN::word;
    constexpr int V = 16 / (int)sizeof(W);
    static_assert(V * sizeof(W) == 16 && (V & (V - 1)) == 0, "a group is one 16-byte load");
    struct alignas(16) Group {
        W w[V];
    };
    // span element i is sample rel0 + i of the call (negative: the carry); groups are counted from the call's input, which
    // is 16-byte aligned, so the first group may begin in front of the span and the last may end behind it
    const long long g0 = (rel0 - (rel0 < 0 ? V - 1 : 0)) / V;  // floor
    const int groups = (int)((rel0 + len - 1) / V - g0) + 1;   // (the span's last sample is never negative)
    for (int g = tid; g < groups; g += kChanThreads) {
        const long long r0 = (g0 + g) * V;
        const int i0 = (int)(r0 - rel0);
        if (i0 >= 0 && i0 + V <= len && r0 >= 0 && r0 + V <= (long long)n_in) {
            // the whole group is span and this call's input (so at or behind the origin): one load, no test per sample
            const Group gr = *reinterpret_cast<const Group *>(in + r0);
#pragma unroll
            for (int j = 0; j < V; j++)
                span[i0 + j] = make_float2(fmt.re(gr.w[j]), fmt.im(gr.w[j]));
        } else {
#pragma unroll 1
            for (int j = 0; j < V; j++) {
                const int i = i0 + j;
                if (i < 0 || i >= len)
                    continue;
                const long long rel = r0 + j;
                float re = 0.f, im = 0.f;  // the stream is preceded by zero samples
                if (first + rel >= origin) {
                    const W w = rel < 0 ? carry[rel + (T - 1)] : in[rel];
                    re = fmt.re(w);
                    im = fmt.im(w);
                }
                span[i] = make_float2(re, im);
            }
        }
    }
}

template <class IN>
__global__ __launch_bounds__(kChanThreads) void k_chan(IN fmt, const typename IN::word *__restrict__ in,
                                                       const typename IN::word *__restrict__ carry, const float2 *__restrict__ nco,
                                                       const float *__restrict__ taps, const int *__restrict__ channels,
                                                       float2 *__restrict__ out, size_t out_stride, long long first, long long origin,
                                                       int n_in, int n_out, int log_m, int D, int T, int span_len)
{
    extern __shared__ __attribute__((aligned(16))) float2 chan_lds[];
    constexpr int J = kChanItemsPerThread;
    const int M = 1 << log_m, log_r = kChanLogItems - log_m, R = 1 << log_r, pitch = M + 1;
    float2 *span = chan_lds;             // [span_len] = [(R - 1) * D + T]
    float2 *img = chan_lds + span_len;   // [R][pitch]
    const int tid = threadIdx.x;
    const int tile0 = blockIdx.x << log_r;  // the tile's first output time, counted inside the call
    const int rn = min(R, n_in / D - tile0);

    // 1. the span: element i is sample tile0 * D - (T - 1) + i of the call
    chan_convert(fmt, in, carry, span, first, origin, (long long)tile0 * D - (T - 1), (rn - 1) * D + T, n_in, T, tid);
    __syncthreads();

    // 2. branch sums: this lane's branch r at output times t0, t0 + dt, ...
    {
        const int r = tid & (M - 1), t0 = tid >> log_m, dt = kChanThreads >> log_m;  // (M = 256: t0 = 0, dt = 1)
        const int P = T >> log_m;
        float2 acc[J];
#pragma unroll
        for (int j = 0; j < J; j++)
            acc[j] = make_float2(0.f, 0.f);
        const float2 *s = span + (T - 1) - r + t0 * D;  // x[n D - r] of the lane's first output time
        const float *h = taps + r;
        const int step = dt * D;
        for (int p = 0; p < P; p++, s -= M, h += M) {
            const float hp = *h;
#pragma unroll
            for (int j = 0; j < J; j++) {
                const float2 y = s[j * step];
                acc[j].x = acc[j].x + (hp * y.x);
                acc[j].y = acc[j].y + (hp * y.y);
            }
        }
        // u[r] is v[(r - n D) mod M], and v[i] is a[bitrev(i)]; n D from the full index (M divides 2^32)
        const uint32_t k0 = (uint32_t)first + (uint32_t)(tile0 + t0) * (uint32_t)D;
#pragma unroll
        for (int j = 0; j < J; j++) {
            const uint32_t v = ((uint32_t)r - (k0 + (uint32_t)(j * step))) & (uint32_t)(M - 1);
            img[(t0 + j * dt) * pitch + (int)(__brev(v) >> (32 - log_m))] = acc[j];
        }
    }

    // 3. the FFT's stages, in place: butterfly b of a stage is row b / (M / 2), pair b mod (M / 2)
    for (int st = 1; st <= log_m; st++) {
        __syncthreads();
        const int half = 1 << (st - 1);
#pragma unroll
        for (int j = 0; j < J / 2; j++) {
            const int b = tid + j * kChanThreads;
            const int row = b >> (log_m - 1), e = b & ((M >> 1) - 1);
            const int q = e & (half - 1);
            float2 *a = img + row * pitch + ((e >> (st - 1)) << st) + q;
            const float2 w = nco[q << (16 - st)];  // q * L / len
            const float2 lo = a[0], hi = a[half];
            const float tre = (w.x * hi.x) - (w.y * hi.y);
            const float tim = (w.x * hi.y) + (w.y * hi.x);
            a[0] = make_float2(lo.x + tre, lo.y + tim);
            a[half] = make_float2(lo.x - tre, lo.y - tim);
        }
    }
    __syncthreads();

    // 4. the selected channels, each as rn consecutive pairs
    for (int it = tid; it < (n_out << log_r); it += kChanThreads) {
        const int t = it & (R - 1), ci = it >> log_r;
        if (t < rn)
            out[(size_t)ci * out_stride + (size_t)(tile0 + t)] = img[t * pitch + channels[ci]];
    }
}

template <class IN>
hipError_t launch_chan_as(IN fmt, const ChanLaunch &l, hipStream_t stream)
{
    using W = typename IN::word;
    const ChanShape s = chan_shape(l.n_channels, l.decimation, l.n_taps);
    if (s.log_m < 0)
        return hipErrorInvalidValue;
    static LdsLimitOnce once;
    const hipError_t e = raise_lds_limit_once(once, {(const void *)k_chan<IN>}, kChanMaxLdsBytes);
    if (e != hipSuccess)
        return e;
    const int m = l.n_in / l.decimation;
    const unsigned tiles = (unsigned)((m + s.tile - 1) / s.tile);
    hipLaunchKernelGGL(k_chan<IN>, dim3(tiles), dim3(kChanThreads), s.lds_bytes, stream, fmt, static_cast<const W *>(l.in),
                       static_cast<const W *>(l.carry), l.nco, l.taps, l.channels, reinterpret_cast<float2 *>(l.out), l.out_stride,
                       l.first, l.origin, l.n_in, l.n_out, s.log_m, l.decimation, l.n_taps, s.span);
    return hipGetLastError();
}

}  // namespace sdr
