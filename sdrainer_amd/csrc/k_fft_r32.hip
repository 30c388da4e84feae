// k_fft_r32.hip — k_fft_r32 (k_fft_r32.h) for float32 input, dense frames: the benchmark's kernel.
#include "k_fft_r32.h"

template hipError_t sdr::launch_fft_r32<sdr::InF32, false>(const sdr::FftLaunch &, sdr::LaunchAt);
