// k_fft_r32_sc16.hip — k_fft_r32 (k_fft_r32.h) for sc16 input (complex int16, sc16.h), dense frames.
#include "k_fft_r32.h"

template hipError_t sdr::launch_fft_r32<sdr::InSc16, false>(const sdr::FftLaunch &, sdr::LaunchAt);
