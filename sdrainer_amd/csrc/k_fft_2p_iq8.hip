// k_fft_2p_iq8.hip — phase A of the two-phase FFT (k_fft_2p_a.h, N = 32768 / 65536) for 8-bit frames (cs8 / cu8, iq8.h),
// plain and windowed.  Phase B is k_fft_2p.hip's.
#include "k_fft_2p_a.h"

template hipError_t sdr::launch_fft_2p<sdr::InFormat::CS8>(const sdr::FftLaunch &, sdr::LaunchAt);
template hipError_t sdr::launch_fft_2p<sdr::InFormat::CU8>(const sdr::FftLaunch &, sdr::LaunchAt);
