// k_ddc.h — the down-converter's kernel bodies (ddc.h, DESIGN.md section 1 "The down-converter"), shared by the two units
// that instantiate them: k_ddc.hip over the four complex input formats (fft_input.h) and k_ddc_real.hip over the four real
// ones.  One wide stream becomes n_bands narrow float32 streams, each mixed to 0 Hz with a table NCO, low-pass filtered by
// the caller's taps and decimated.  The arithmetic is a contract, bit for bit (tests/ddc_ref.py is its NumPy restatement):
// per sample p = (k * step) mod L from the full sample index, (c, s) = NCO[p],
//     yre = (re * c) + (im * s)        yim = (im * c) - (re * s)
// and per output n, for re and im alike,  acc = +0;  for j = 0 .. T-1:  acc = acc + (h[j] * y[n D - j])  - every product and
// every sum rounded on its own (the library is built with -ffp-contract=off), subnormals kept.
//
// An input trait IN names the word one sample is read as and gives its float32 (re, im); a real format's im is +0.0f and
// goes through the same two formulas (0 * s is -0 for a negative s, and a NaN or Inf sample makes both outputs NaN: no
// product is skipped).
//
// A workgroup takes one tile of outputs of one band, chunk by chunk (ddc.h): all its lanes convert and mix the chunk's input
// span once into the polyphase LDS image, then lane l accumulates outputs l and l + threads of the chunk.  The tap index is
// wave-uniform: h[j] and the image row are scalar, a lane's LDS address is its column plus a scalar.  Workgroups of the same
// tile are neighbours in the grid (band is the fast index), so the bands' reads of one input span meet in the caches.
#pragma once
#include <type_traits>

#include "ddc.h"
#include "sdr_device.h"

namespace sdr {

// R outputs per lane: columns col[r] of the image (a lane without an r-th output reads its first again and stores nothing)
template <int R>
__device__ __forceinline__ void ddc_filter(const float2 *__restrict__ img, const float *__restrict__ taps, int D, int T, int width,
                                           const int (&col)[R], float2 (&acc)[R])
{
#pragma unroll
    for (int r = 0; r < R; r++)
        acc[r] = make_float2(0.f, 0.f);
    // tap j meets span element q = T - 1 - j of output 0: row q mod D, column q div D; j ascending walks the rows down
    int j = 0;
    int row = (T - 1) % D;
    for (int c = (T - 1) / D; c >= 0; c--) {
        const float2 *p = img + row * width + c;
        for (; row >= 0; row--, j++, p -= width) {
            const float h = taps[j];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float2 y = p[col[r]];
                acc[r].x = acc[r].x + (h * y.x);
                acc[r].y = acc[r].y + (h * y.y);
            }
        }
        row = D - 1;
    }
}

// samples per 16-byte load of a trait that asks for wide loads (IN::kWide); 1: one word per lane
template <class IN, class = void>
struct DdcWide {
    static constexpr int value = 1;
};
template <class IN>
struct DdcWide<IN, std::void_t<decltype(IN::kWide)>> {
    static constexpr int value = IN::kWide;
};

// The mix of a chunk's span with 16-byte loads: a lane takes the V samples at one 16-byte place of the call's input (in is
// 16-byte aligned), so a group may begin in front of the span.  A group that lies inside the span and the call's input is
// one load, and its V table reads and image stores are independent of each other; one that crosses an end of the span,
// touches the carry (rel < 0) or the input's end is mixed sample by sample with every test of the one-word loop.  The
// groups are dealt to the lanes in whole rounds; a last round that the one-word loop does in a single pass is left to it.
// Returns the span elements mixed, counted from the span's start: the one-word loop goes on from there.
template <class IN>
__device__ __forceinline__ int ddc_mix_wide(IN fmt, const typename IN::word *__restrict__ in, const typename IN::word *__restrict__ carry,
                                             const float2 *__restrict__ nco, float2 *__restrict__ img, long long first, long long origin,
                                             long long rel0, int span, int n_in, int D, int T, int width, uint32_t step, int tid, int nt)
{
    using W = typename IN::word;
    constexpr int V = DdcWide<IN>::value;
    static_assert(V * sizeof(W) == 16 && (V & (V - 1)) == 0, "a group is one 16-byte load");
    struct alignas(16) Group {
        W w[V];
    };
    const long long g0 = (rel0 - (rel0 < 0 ? V - 1 : 0)) / V;  // floor: the group that holds the span's first sample
    const int groups = (int)((rel0 + span - 1) / V + 1 - g0);  // (the span's last sample is never negative)
    int rounds = groups / nt;
    if ((groups - rounds * nt) * V > nt)
        rounds++;
    const int i_stop = (int)((g0 + (long long)rounds * nt) * V - rel0);  // the first span element behind the rounds' groups
    const int bias = (V + D - 1) / D;                           // whole columns that make a group's first element positive
    const int stride = nt * V;
    const int drow = stride % D, dcol = stride / D;
    long long r0 = (g0 + tid) * V;  // the group's first sample, counted inside the call
    int i0 = (int)(r0 - rel0);      // its span element, > -V
    int row0 = (i0 + bias * D) % D, col0 = (i0 + bias * D) / D - bias;
    for (; i0 < i_stop; r0 += stride, i0 += stride) {
        int row = row0, col = col0;
        if (i0 >= 0 && i0 + V <= span && r0 >= 0 && r0 + V <= (long long)n_in) {
            // the whole group is span and this call's input (so at or behind the origin): one load, no test per sample
            const Group g = *reinterpret_cast<const Group *>(in + r0);
            const uint32_t k0 = (uint32_t)(first + r0);
#pragma unroll
            for (int j = 0; j < V; j++) {
                const float re = fmt.re(g.w[j]), im = fmt.im(g.w[j]);
                const float2 cs = nco[((k0 + (uint32_t)j) * step) & (uint32_t)(kDdcNco - 1)];
                img[row * width + col] = make_float2((re * cs.x) + (im * cs.y), (im * cs.x) - (re * cs.y));
                if (++row == D) {
                    row = 0;
                    col++;
                }
            }
        } else {
            // a group across the span's start or end, the carry or the input's end: sample by sample, as the one-word loop
#pragma unroll 1
            for (int j = 0; j < V; j++) {
                const long long rel = r0 + j, k = first + rel;
                if (i0 + j >= 0 && i0 + j < span) {
                    float re = 0.f, im = 0.f;  // the stream is preceded by zero samples
                    if (k >= origin) {
                        const W w = rel < 0 ? carry[rel + (T - 1)] : in[rel];
                        re = fmt.re(w);
                        im = fmt.im(w);
                    }
                    const float2 cs = nco[((uint32_t)k * step) & (uint32_t)(kDdcNco - 1)];
                    img[row * width + col] = make_float2((re * cs.x) + (im * cs.y), (im * cs.x) - (re * cs.y));
                }
                if (++row == D) {
                    row = 0;
                    col++;
                }
            }
        }
        row0 += drow;
        col0 += dcol;
        if (row0 >= D) {
            row0 -= D;
            col0++;
        }
    }
    return max(0, min(span, i_stop));
}

template <class IN>
__global__ __launch_bounds__(kDdcMaxThreads) void k_ddc(IN fmt, const typename IN::word *__restrict__ in,
                                                        const typename IN::word *__restrict__ carry, const float2 *__restrict__ nco,
                                                        const float *__restrict__ taps, float2 *__restrict__ out, size_t out_stride,
                                                        long long first, long long origin, int n_in, int n_bands, int D, int T,
                                                        int chunk, int width, DdcSteps steps)
{
    extern __shared__ float2 ddc_img[];
    float2 *img = ddc_img;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int band = blockIdx.x % n_bands;
    const int tile0 = (blockIdx.x / n_bands) * kDdcTileOutputs;  // the tile's first output, counted inside the call
    const int tile_n = min(kDdcTileOutputs, n_in / D - tile0);
    const uint32_t step = (uint16_t)steps.step[band];  // two's complement: (k * step) mod 2^16 needs the low 16 bits only
    float2 *o = out + (size_t)band * out_stride + tile0;
    const int drow = nt % D, dcol = nt / D;

    for (int c0 = 0; c0 < tile_n; c0 += chunk) {
        const int cn = min(chunk, tile_n - c0);
        const int span = (cn - 1) * D + T;
        // span element i is input sample rel0 + i of the call (negative: the carry), stream sample first + rel0 + i
        const long long rel0 = (long long)(tile0 + c0) * D - (T - 1);
        int i = tid;
        if constexpr (DdcWide<IN>::value > 1)
            i += ddc_mix_wide(fmt, in, carry, nco, img, first, origin, rel0, span, n_in, D, T, width, step, tid, nt);
        int row = i % D, col = i / D;
        for (; i < span; i += nt) {
            const long long rel = rel0 + i, k = first + rel;
            float re = 0.f, im = 0.f;  // the stream is preceded by zero samples
            if (k >= origin) {
                const typename IN::word w = rel < 0 ? carry[rel + (T - 1)] : in[rel];
                re = fmt.re(w);
                im = fmt.im(w);
            }
            const float2 cs = nco[((uint32_t)k * step) & (uint32_t)(kDdcNco - 1)];
            img[row * width + col] = make_float2((re * cs.x) + (im * cs.y), (im * cs.x) - (re * cs.y));
            row += drow;
            col += dcol;
            if (row >= D) {
                row -= D;
                col++;
            }
        }
        __syncthreads();
        if (tid < cn) {
            if (cn > nt) {
                const bool second = tid + nt < cn;
                const int colr[2] = {tid, second ? tid + nt : tid};
                float2 acc[2];
                ddc_filter<2>(img, taps, D, T, width, colr, acc);
                o[c0 + tid] = acc[0];
                if (second)
                    o[c0 + tid + nt] = acc[1];
            } else {
                const int colr[1] = {tid};
                float2 acc[1];
                ddc_filter<1>(img, taps, D, T, width, colr, acc);
                o[c0 + tid] = acc[0];
            }
        }
        __syncthreads();
    }
}

// the next carry, by raw words: W is any type of the sample's size
template <class W>
__global__ __launch_bounds__(256) void k_ddc_carry(const W *__restrict__ carry_in, const W *__restrict__ in, int n_in, int keep,
                                                   W *__restrict__ carry_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= keep)
        return;
    const int s = i + (n_in - keep);  // the sample's place in this call's input; negative: it was carried already
    carry_out[i] = s >= 0 ? in[s] : carry_in[s + keep];
}

template <class IN>
hipError_t launch_ddc_as(IN fmt, const DdcLaunch &l, hipStream_t stream)
{
    using W = typename IN::word;
    const DdcShape s = ddc_shape(l.decimation, l.n_taps);
    static LdsLimitOnce once;
    const hipError_t e = raise_lds_limit_once(once, {(const void *)k_ddc<IN>}, kDdcMaxLdsBytes);
    if (e != hipSuccess)
        return e;
    const int m = l.n_in / l.decimation;
    const unsigned tiles = (unsigned)((m + kDdcTileOutputs - 1) / kDdcTileOutputs);
    hipLaunchKernelGGL(k_ddc<IN>, dim3(tiles * (unsigned)l.n_bands), dim3((unsigned)s.threads), s.lds_bytes, stream, fmt,
                       static_cast<const W *>(l.in), static_cast<const W *>(l.carry), l.nco, l.taps, reinterpret_cast<float2 *>(l.out),
                       l.out_stride, l.first, l.origin, l.n_in, l.n_bands, l.decimation, l.n_taps, s.chunk, s.width, l.steps);
    return hipGetLastError();
}

template <class W>
hipError_t launch_carry_as(const void *carry_in, const void *in, int n_in, int keep, void *carry_out, hipStream_t stream)
{
    hipLaunchKernelGGL(k_ddc_carry<W>, dim3((unsigned)((keep + 255) / 256)), dim3(256), 0, stream, static_cast<const W *>(carry_in),
                       static_cast<const W *>(in), n_in, keep, static_cast<W *>(carry_out));
    return hipGetLastError();
}

// k_ddc_real.hip: what launch_ddc and launch_ddc_carry (k_ddc.hip) hand the real formats and the one-byte sample to
hipError_t launch_ddc_real(const DdcLaunch &l, hipStream_t stream);
hipError_t launch_ddc_carry_byte(const void *carry_in, const void *in, int n_in, int keep, void *carry_out, hipStream_t stream);

}  // namespace sdr
