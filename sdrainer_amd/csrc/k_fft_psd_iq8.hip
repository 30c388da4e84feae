// k_fft_psd_iq8.hip — k_fft_psd (k_fft_psd.h) for 8-bit input (cs8 / cu8, iq8.h), without a window and with one.
#include "k_fft_psd.h"

template hipError_t sdr::launch_fft_psd<sdr::InIq8, false>(const sdr::FftLaunch &, sdr::LaunchAt);
template hipError_t sdr::launch_fft_psd<sdr::InIq8, true>(const sdr::FftLaunch &, sdr::LaunchAt);
