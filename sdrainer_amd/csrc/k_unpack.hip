// k_unpack.hip — source-side wire format on the device: KiwiSDR "SND" frames carry
// IQ as big-endian int16 pairs (kiwi/client.go:284-308 decodeIQMessage / decodeIQBytes:
// float32(int16(be16)) / float32(math.MaxInt16)).  Unpacking in HBM halves the PCIe bytes of that
// source: the raw payload is what gets uploaded.
#include <hip/hip_runtime.h>

#include "iq8.h"
#include "sc16.h"
#include "sdr_device.h"

namespace sdr {

__device__ __forceinline__ float be16_to_f32(uint32_t lo_byte_first)
{
    // bytes b0 b1 (network order): value = int16(b0 << 8 | b1)
    const uint32_t v = ((lo_byte_first & 0xffu) << 8) | ((lo_byte_first >> 8) & 0xffu);
    return __fdiv_rn((float)(int16_t)v, 32767.0f);  // correctly rounded float32 division, as Go's
}

// 8 payload bytes -> 4 floats per thread (16-byte stores)
__global__ __launch_bounds__(256) void k_unpack_be16(const uint8_t *__restrict__ raw, float *__restrict__ out,
                                                     size_t n_values)
{
    const size_t i4 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i = i4 * 4;
    if (i >= n_values)
        return;
    if (i + 4 <= n_values) {
        const uint2 w = *reinterpret_cast<const uint2 *>(raw + 2 * i);  // staging buffers are 8-byte aligned
        float4 f;
        f.x = be16_to_f32(w.x & 0xffffu);
        f.y = be16_to_f32(w.x >> 16);
        f.z = be16_to_f32(w.y & 0xffffu);
        f.w = be16_to_f32(w.y >> 16);
        *reinterpret_cast<float4 *>(out + i) = f;
    } else {
        for (size_t k = i; k < n_values; k++)
            out[k] = be16_to_f32((uint32_t)raw[2 * k] | ((uint32_t)raw[2 * k + 1] << 8));
    }
}

hipError_t launch_unpack_be16(const uint8_t *raw, float *out, size_t n_values, hipStream_t stream)
{
    if (n_values == 0)
        return hipSuccess;
    const size_t threads = (n_values + 3) / 4;
    hipLaunchKernelGGL(k_unpack_be16, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, raw, out, n_values);
    return hipGetLastError();
}

// sdr_push_iq_sc16: little-endian int16 values (sc16) -> float32, 4 values per thread (8-byte loads, 16-byte stores);
// the conversion is the one the sc16 FFT kernels use (sc16.h)
__global__ __launch_bounds__(256) void k_unpack_sc16(const int16_t *__restrict__ raw, float *__restrict__ out, size_t n_values)
{
    const size_t i4 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i = i4 * 4;
    if (i >= n_values)
        return;
    if (i + 4 <= n_values) {
        const uint2 w = *reinterpret_cast<const uint2 *>(raw + i);  // staging buffers are 8-byte aligned
        float4 f;
        f.x = sc16::re_of(w.x);
        f.y = sc16::im_of(w.x);
        f.z = sc16::re_of(w.y);
        f.w = sc16::im_of(w.y);
        *reinterpret_cast<float4 *>(out + i) = f;
    } else {
        for (size_t k = i; k < n_values; k++)
            out[k] = sc16::to_f32(raw[k]);
    }
}

hipError_t launch_unpack_sc16(const int16_t *raw, float *out, size_t n_values, hipStream_t stream)
{
    if (n_values == 0)
        return hipSuccess;
    const size_t threads = (n_values + 3) / 4;
    hipLaunchKernelGGL(k_unpack_sc16, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, raw, out, n_values);
    return hipGetLastError();
}

// sdr_push_iq8: cs8 / cu8 bytes (iq8.h) -> float32, 8 values per thread (one 8-byte load, two 16-byte stores); the
// conversion is the one the 8-bit FFT kernels use.  flip / c: iq8::Format (flip holds the mask of two bytes, as a sample's)
__global__ __launch_bounds__(256) void k_unpack_iq8(const uint8_t *__restrict__ raw, float *__restrict__ out, size_t n_values, unsigned flip, float c)
{
    const size_t i8 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t i = i8 * 8;
    if (i >= n_values)
        return;
    const iq8::Format f{flip, c};
    if (i + 8 <= n_values) {
        const uint2 w = *reinterpret_cast<const uint2 *>(raw + i);  // staging buffers are 8-byte aligned
        float4 a, b;
        a.x = iq8::re_of(w.x, f);
        a.y = iq8::im_of(w.x, f);
        a.z = iq8::re_of(w.x >> 16, f);
        a.w = iq8::im_of(w.x >> 16, f);
        b.x = iq8::re_of(w.y, f);
        b.y = iq8::im_of(w.y, f);
        b.z = iq8::re_of(w.y >> 16, f);
        b.w = iq8::im_of(w.y >> 16, f);
        *reinterpret_cast<float4 *>(out + i) = a;
        *reinterpret_cast<float4 *>(out + i + 4) = b;
    } else {
        for (size_t k = i; k < n_values; k++)
            out[k] = iq8::re_of(raw[k], f);
    }
}

hipError_t launch_unpack_iq8(const uint8_t *raw, float *out, size_t n_values, bool cu8, hipStream_t stream)
{
    if (n_values == 0)
        return hipSuccess;
    const size_t threads = (n_values + 7) / 8;
    const iq8::Format f = iq8::format_of(cu8);
    hipLaunchKernelGGL(k_unpack_iq8, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, raw, out, n_values, f.flip, f.c);
    return hipGetLastError();
}

}  // namespace sdr
