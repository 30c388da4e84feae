// k_iq_sums.hip — the exact sums of a call's raw samples (include/sdrainer_hip.h "IQ correction", iq_sums_dev.h): one
// memory-bound reduction over the input on the object's stream, behind the call's main kernel, and a one-workgroup pass
// that adds the call's total to the object's record.
//
// k_iq_sums_iq8 / k_iq_sums_sc16: a lane reads 16 bytes per load (8 byte-pair samples, 4 sc16 samples), kIqSumsGroupsPerLane
// of them a wave's width apart, so a wave's load is 1 KB of consecutive input; the grid follows from the input's length.
// The lane that meets the group the samples do not fill takes it word by word.  8-bit values are summed as b = byte ^ flip,
// 0 .. 255 for both formats (host/iq_sums.h): a lane adds at most 128 products below 2^16 to an int32.  sc16 squares go to
// 64-bit accumulators.  Then a wave reduction, the four waves through LDS, and one row of five int64 per workgroup in the
// partial slab.  k_iq_sums_finish sums the slab in a fixed order, turns b into the unit u = a b + c and adds to the record:
// integers only, one writer, so the bits depend on no schedule.
#include "iq_sums_dev.h"

namespace sdr {
namespace {

using Red = long long[kIqSumsThreads / 64][kIqSumsValues];

// every lane's v summed over the workgroup: red[w][k] holds wave w's totals when this returns
__device__ __forceinline__ void iq_block_totals(long long (&v)[kIqSumsValues], Red &red)
{
#pragma unroll
    for (int k = 0; k < kIqSumsValues; k++)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
            v[k] += __shfl_down(v[k], off, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < kIqSumsValues; k++)
            red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
}

__device__ __forceinline__ long long iq_red_total(const Red &red, int k)
{
    long long t = 0;
#pragma unroll
    for (int w = 0; w < kIqSumsThreads / 64; w++)
        t += red[w][k];
    return t;
}

// two samples of a dword whose bytes are b already (I0 Q0 I1 Q1; the ragged end passes one sample and zeros)
__device__ __forceinline__ void iq8_add(uint32_t w, uint32_t (&s)[kIqSumsValues])
{
    const uint32_t i = w & 0x00ff00ffu, q = (w >> 8) & 0x00ff00ffu;
    s[0] = __builtin_amdgcn_udot4(i, 0x00010001u, s[0], false);
    s[1] = __builtin_amdgcn_udot4(q, 0x00010001u, s[1], false);
    s[2] = __builtin_amdgcn_udot4(i, i, s[2], false);
    s[3] = __builtin_amdgcn_udot4(q, q, s[3], false);
    s[4] = __builtin_amdgcn_udot4(i, q, s[4], false);
}

__global__ __launch_bounds__(kIqSumsThreads) void k_iq_sums_iq8(const uint4 *__restrict__ in, long long n, uint32_t flip,
                                                                 long long *__restrict__ part)
{
    __shared__ Red red;
    const long long whole = n >> 3;  // groups of eight samples
    const int tail = (int)(n & 7);
    const uint32_t flip2 = flip | (flip << 16);
    uint32_t s[kIqSumsValues] = {0, 0, 0, 0, 0};
    long long g = (long long)blockIdx.x * kIqSumsBlockGroups + threadIdx.x;
#pragma unroll 4
    for (int j = 0; j < kIqSumsGroupsPerLane; j++, g += kIqSumsThreads) {
        if (g < whole) {
            const uint4 v = in[g];
            iq8_add(v.x ^ flip2, s);
            iq8_add(v.y ^ flip2, s);
            iq8_add(v.z ^ flip2, s);
            iq8_add(v.w ^ flip2, s);
        } else if (g == whole) {
            const uint16_t *w = reinterpret_cast<const uint16_t *>(in + g);
            for (int t = 0; t < tail; t++)
                iq8_add((uint32_t)w[t] ^ flip, s);
        }
    }
    long long v[kIqSumsValues];
#pragma unroll
    for (int k = 0; k < kIqSumsValues; k++)
        v[k] = (long long)s[k];
    iq_block_totals(v, red);
    if (threadIdx.x < kIqSumsValues)
        part[(size_t)blockIdx.x * kIqSumsValues + threadIdx.x] = iq_red_total(red, (int)threadIdx.x);
}

// one sc16 sample: I in the low half, Q in the high half
__device__ __forceinline__ void sc16_add(uint32_t w, int (&lin)[2], long long (&sq)[3])
{
    const int i = (int)(short)(w & 0xffffu), q = (int)w >> 16;
    lin[0] += i;
    lin[1] += q;
    sq[0] += (long long)i * i;
    sq[1] += (long long)q * q;
    sq[2] += (long long)i * q;
}

__global__ __launch_bounds__(kIqSumsThreads) void k_iq_sums_sc16(const uint4 *__restrict__ in, long long n, long long *__restrict__ part)
{
    __shared__ Red red;
    const long long whole = n >> 2;  // groups of four samples
    const int tail = (int)(n & 3);
    int lin[2] = {0, 0};  // at most 64 values of 16 bits
    long long sq[3] = {0, 0, 0};
    long long g = (long long)blockIdx.x * kIqSumsBlockGroups + threadIdx.x;
#pragma unroll 4
    for (int j = 0; j < kIqSumsGroupsPerLane; j++, g += kIqSumsThreads) {
        if (g < whole) {
            const uint4 v = in[g];
            sc16_add(v.x, lin, sq);
            sc16_add(v.y, lin, sq);
            sc16_add(v.z, lin, sq);
            sc16_add(v.w, lin, sq);
        } else if (g == whole) {
            const uint32_t *w = reinterpret_cast<const uint32_t *>(in + g);
            for (int t = 0; t < tail; t++)
                sc16_add(w[t], lin, sq);
        }
    }
    long long v[kIqSumsValues] = {lin[0], lin[1], sq[0], sq[1], sq[2]};
    iq_block_totals(v, red);
    if (threadIdx.x < kIqSumsValues)
        part[(size_t)blockIdx.x * kIqSumsValues + threadIdx.x] = iq_red_total(red, (int)threadIdx.x);
}

// the call's total: the slab's rows in a fixed order, b -> u, and the record's one writer
__global__ __launch_bounds__(kIqSumsThreads) void k_iq_sums_finish(const long long *__restrict__ part, int blocks, IqUnit unit, long long n,
                                                                    long long *__restrict__ rec)
{
    __shared__ Red red;
    long long v[kIqSumsValues] = {0, 0, 0, 0, 0};
    for (int b = (int)threadIdx.x; b < blocks; b += kIqSumsThreads)
#pragma unroll
        for (int k = 0; k < kIqSumsValues; k++)
            v[k] += part[(size_t)b * kIqSumsValues + k];
    iq_block_totals(v, red);
    if (threadIdx.x == 0) {
        const IqRawSums u = iq_unit_sums(IqRawSums{iq_red_total(red, 0), iq_red_total(red, 1), iq_red_total(red, 2), iq_red_total(red, 3),
                                                   iq_red_total(red, 4)}, unit, n);
        rec[0] += u.i;
        rec[1] += u.q;
        rec[2] += u.ii;
        rec[3] += u.qq;
        rec[4] += u.iq;
    }
}

constexpr size_t kRecBytes = sizeof(long long) * kIqSumsValues;

}  // namespace

hipError_t iq_sums_enable(IqSums &s, int fmt, int max_in_samples, bool on, hipStream_t stream)
{
    if (!iq_sums_format(fmt))
        return hipErrorInvalidValue;
    if (on && !s.d_rec) {
        long long *rec = nullptr, *part = nullptr;
        hipError_t e = hipMalloc((void **)&rec, kRecBytes);
        if (e != hipSuccess)
            return e;
        e = hipMalloc((void **)&part, kRecBytes * (size_t)iq_sums_blocks(fmt, max_in_samples));
        if (e != hipSuccess) {
            (void)hipFree(rec);
            return e;
        }
        s.d_rec = rec;
        s.d_part = part;
    }
    if (s.d_rec) {
        const hipError_t e = hipMemsetAsync(s.d_rec, 0, kRecBytes, stream);
        if (e != hipSuccess)
            return e;
    }
    s.count.clear();
    s.on = on;
    return hipSuccess;
}

hipError_t iq_sums_add(IqSums &s, int fmt, const void *in, int n_in, hipStream_t stream)
{
    if (!s.on || !iq_sums_format(fmt))
        return hipErrorInvalidValue;
    if (!s.count.accept(n_in))
        return hipSuccess;
    const unsigned blocks = (unsigned)iq_sums_blocks(fmt, n_in);
    const uint4 *p = static_cast<const uint4 *>(in);
    if (fmt == SDR_DDC_SC16)
        hipLaunchKernelGGL(k_iq_sums_sc16, dim3(blocks), dim3(kIqSumsThreads), 0, stream, p, (long long)n_in, s.d_part);
    else
        hipLaunchKernelGGL(k_iq_sums_iq8, dim3(blocks), dim3(kIqSumsThreads), 0, stream, p, (long long)n_in,
                           fmt == SDR_DDC_CS8 ? 0x8080u : 0u, s.d_part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_iq_sums_finish, dim3(1), dim3(kIqSumsThreads), 0, stream, s.d_part, (int)blocks, iq_unit(fmt), (long long)n_in,
                       s.d_rec);
    return hipGetLastError();
}

hipError_t iq_sums_read(IqSums &s, sdr_iq_sums *out, hipStream_t stream)
{
    if (!s.on || !out)
        return hipErrorInvalidValue;
    long long rec[kIqSumsValues];
    hipError_t e = hipMemcpyAsync(rec, s.d_rec, kRecBytes, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(stream);
    if (e == hipSuccess)
        e = hipMemsetAsync(s.d_rec, 0, kRecBytes, stream);
    if (e != hipSuccess)
        return e;
    *out = sdr_iq_sums{s.count.n, rec[0], rec[1], rec[2], rec[3], rec[4], s.count.skipped, 0};
    s.count.clear();
    return hipSuccess;
}

void iq_sums_free(IqSums &s)
{
    (void)hipFree(s.d_rec);
    (void)hipFree(s.d_part);
    s = IqSums{};
}

}  // namespace sdr
