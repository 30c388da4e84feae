// k_fft_r32_hop_iq8.hip — k_fft_r32 (k_fft_r32.h) for 8-bit input (cs8 / cu8), overlapped frames (a frame stride below N).
#include "k_fft_r32.h"

template hipError_t sdr::launch_fft_r32<sdr::InIq8, true>(const sdr::FftLaunch &, sdr::LaunchAt);
