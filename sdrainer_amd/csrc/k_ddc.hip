// k_ddc.hip — the down-converter's kernel (ddc.h, DESIGN.md section 1 "The down-converter"): one wide stream in any of
// the four input formats (fft_input.h) becomes n_bands narrow float32 streams, each mixed to 0 Hz with a table NCO,
// low-pass filtered by the caller's taps and decimated.  The arithmetic is a contract, bit for bit (tests/ddc_ref.py is its
// NumPy restatement): per sample p = (k * step) mod L from the full sample index, (c, s) = NCO[p],
//     yre = (re * c) + (im * s)        yim = (im * c) - (re * s)
// and per output n, for re and im alike,  acc = +0;  for j = 0 .. T-1:  acc = acc + (h[j] * y[n D - j])  - every product and
// every sum rounded on its own (the library is built with -ffp-contract=off), subnormals kept.
//
// A workgroup takes one tile of outputs of one band, chunk by chunk (ddc.h): all its lanes convert and mix the chunk's input
// span once into the polyphase LDS image, then lane l accumulates outputs l and l + threads of the chunk.  The tap index is
// wave-uniform: h[j] and the image row are scalar, a lane's LDS address is its column plus a scalar.  Workgroups of the same
// tile are neighbours in the grid (band is the fast index), so the bands' reads of one input span meet in the caches.
#include "ddc.h"
#include "fft_input.h"

namespace sdr {
namespace {

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
        int row = tid % D, col = tid / D;
        for (int i = tid; i < span; i += nt) {
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

}  // namespace

hipError_t launch_ddc(const DdcLaunch &l, hipStream_t stream)
{
    switch (l.fmt) {
    case SDR_DDC_F32: return launch_ddc_as(InF32{}, l, stream);
    case SDR_DDC_SC16: return launch_ddc_as(InSc16{}, l, stream);
    case SDR_DDC_CS8: return launch_ddc_as(InIq8{iq8::format_of(false)}, l, stream);
    case SDR_DDC_CU8: return launch_ddc_as(InIq8{iq8::format_of(true)}, l, stream);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_ddc_carry(int fmt, const void *carry_in, const void *in, int n_in, int n_taps, void *carry_out, hipStream_t stream)
{
    const int keep = n_taps - 1;
    if (keep <= 0)
        return hipSuccess;
    switch (fmt) {
    case SDR_DDC_F32: return launch_carry_as<InF32::word>(carry_in, in, n_in, keep, carry_out, stream);
    case SDR_DDC_SC16: return launch_carry_as<InSc16::word>(carry_in, in, n_in, keep, carry_out, stream);
    case SDR_DDC_CS8:
    case SDR_DDC_CU8: return launch_carry_as<InIq8::word>(carry_in, in, n_in, keep, carry_out, stream);
    }
    return hipErrorInvalidValue;
}

}  // namespace sdr
