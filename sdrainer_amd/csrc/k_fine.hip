// k_fine.hip — the fine converter's two kernels (fine.h, include/sdrainer_hip.h "fine converter").  k_fine is the
// down-converter's kernel (k_ddc.h, whose contract and bodies it shares by inclusion: the polyphase LDS image of ddc_shape,
// the chunks, the wave-uniform tap loop ddc_filter) with one difference: a workgroup computes one tile of one band from
// in + input[band] * in_stride and that input's carry instead of from the single wide stream.  The arithmetic per sample
// and per output is k_ddc<InF32>'s, operation for operation, so a band equals a one-band SDR_DDC_F32 down-converter fed
// that stream, bit for bit.  k_fine_carry forms the next carry of all n_inputs streams in one launch.
//
// A float32 pair per lane is an 8-byte load; the 16-byte groups of k_ddc.h's ddc_mix_wide are not taken here: the span is
// mixed once per chunk while the tap loop runs T times per output, and the one-word loop has no group that can straddle the
// carry, the span's ends or an input's end.
//
// Workgroups of one tile are neighbours in the grid (band is the fast index): bands that read one input meet in the caches.
#include "fine.h"
#include "k_ddc.h"

namespace sdr {

__global__ __launch_bounds__(kDdcMaxThreads) void k_fine(const float2 *__restrict__ in, size_t in_stride, const float2 *__restrict__ carry,
                                                         const float2 *__restrict__ nco, const float *__restrict__ taps,
                                                         float2 *__restrict__ out, size_t out_stride, long long first, long long origin,
                                                         int n_in, int n_bands, int D, int T, int chunk, int width, FineMap map)
{
    extern __shared__ float2 fine_img[];
    float2 *img = fine_img;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int band = blockIdx.x % n_bands;
    const int tile0 = (blockIdx.x / n_bands) * kDdcTileOutputs;  // the tile's first output, counted inside the call
    const int tile_n = min(kDdcTileOutputs, n_in / D - tile0);
    const uint32_t step = (uint16_t)map.step[band];  // two's complement: (k * step) mod 2^16 needs the low 16 bits only
    const size_t input = map.input[band];
    const float2 *x = in + input * in_stride;          // this band's stream
    const float2 *hist = carry + input * (size_t)(T - 1);  // and the T - 1 samples in front of it
    float2 *o = out + (size_t)band * out_stride + tile0;
    const int drow = nt % D, dcol = nt / D;

    for (int c0 = 0; c0 < tile_n; c0 += chunk) {
        const int cn = min(chunk, tile_n - c0);
        const int span = (cn - 1) * D + T;
        // span element i is input sample rel0 + i of the call (negative: the carry), stream sample first + rel0 + i
        const long long rel0 = (long long)(tile0 + c0) * D - (T - 1);
        int i = tid;
        int row = i % D, col = i / D;
        for (; i < span; i += nt) {
            const long long rel = rel0 + i, k = first + rel;
            float re = 0.f, im = 0.f;  // the stream is preceded by zero samples
            if (k >= origin) {
                const float2 w = rel < 0 ? hist[rel + (T - 1)] : x[rel];
                re = w.x;
                im = w.y;
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

// the next carry of every input: blockIdx.y is the input
__global__ __launch_bounds__(256) void k_fine_carry(const float2 *__restrict__ carry_in, const float2 *__restrict__ in, size_t in_stride,
                                                    int n_in, int keep, float2 *__restrict__ carry_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= keep)
        return;
    const size_t input = blockIdx.y;
    const int s = i + (n_in - keep);  // the sample's place in this call's input; negative: it was carried already
    carry_out[input * (size_t)keep + i] = s >= 0 ? in[input * in_stride + s] : carry_in[input * (size_t)keep + (s + keep)];
}

hipError_t launch_fine(const FineLaunch &l, hipStream_t stream)
{
    const DdcShape s = ddc_shape(l.decimation, l.n_taps);
    static LdsLimitOnce once;
    const hipError_t e = raise_lds_limit_once(once, {(const void *)k_fine}, kDdcMaxLdsBytes);
    if (e != hipSuccess)
        return e;
    const int m = l.n_in / l.decimation;
    const unsigned tiles = (unsigned)((m + kDdcTileOutputs - 1) / kDdcTileOutputs);
    hipLaunchKernelGGL(k_fine, dim3(tiles * (unsigned)l.n_bands), dim3((unsigned)s.threads), s.lds_bytes, stream, l.in, l.in_stride,
                       l.carry, l.nco, l.taps, reinterpret_cast<float2 *>(l.out), l.out_stride, l.first, l.origin, l.n_in, l.n_bands,
                       l.decimation, l.n_taps, s.chunk, s.width, l.map);
    return hipGetLastError();
}

hipError_t launch_fine_carry(const float2 *carry_in, const float2 *in, size_t in_stride, int n_in, int n_inputs, int n_taps,
                             float2 *carry_out, hipStream_t stream)
{
    const int keep = n_taps - 1;
    if (keep <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_fine_carry, dim3((unsigned)((keep + 255) / 256), (unsigned)n_inputs), dim3(256), 0, stream, carry_in, in,
                       in_stride, n_in, keep, carry_out);
    return hipGetLastError();
}

}  // namespace sdr
