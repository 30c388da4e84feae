// k_fft_psd.hip — k_fft_psd (k_fft_psd.h) for float32 and sc16 input, without a window.
#if defined(SDR_FFT_CLOCK_LIB)
// diagnostic LIBRARY build (tools/build_abl.sh fftclk "-DSDR_FFT_CLOCK -DSDR_FFT_CLOCK_LIB", tools/insitu_fft.py): the
// per-workgroup spans of this unit's float32 launches inside the running pipeline.  Here and in no other unit.
#define SDR_FFT_CLOCK_LIB_UNIT
#include <hip/hip_runtime.h>
namespace sdr {
__device__ unsigned long long g_fft_clock[2];
__device__ unsigned long long g_fft_wg[2048][4];
extern "C" __attribute__((visibility("default"))) int sdr_debug_fft_wg(unsigned long long *out)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fft_wg), sizeof(g_fft_wg));
}
}  // namespace sdr
#endif
#include "k_fft_psd.h"

template hipError_t sdr::launch_fft_psd<sdr::InF32, false>(const sdr::FftLaunch &, sdr::LaunchAt);
template hipError_t sdr::launch_fft_psd<sdr::InSc16, false>(const sdr::FftLaunch &, sdr::LaunchAt);
