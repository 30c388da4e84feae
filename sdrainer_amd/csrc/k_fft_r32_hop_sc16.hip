// k_fft_r32_hop_sc16.hip — k_fft_r32 (k_fft_r32.h) for sc16 input, overlapped frames (a frame stride below N).
#include "k_fft_r32.h"

template hipError_t sdr::launch_fft_r32<sdr::InSc16, true>(const sdr::FftLaunch &, sdr::LaunchAt);
