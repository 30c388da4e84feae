// k_fft_r32_hop.hip — k_fft_r32 (k_fft_r32.h) for float32 input, overlapped frames (a frame stride below N).
#include "k_fft_r32.h"

template hipError_t sdr::launch_fft_r32<sdr::InF32, true>(const sdr::FftLaunch &, sdr::LaunchAt);
