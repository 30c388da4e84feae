// k_fft_psd_win.hip — k_fft_psd (k_fft_psd.h) for float32 and sc16 input with a window on the frames (sdr_set_window).
#include "k_fft_psd.h"

template hipError_t sdr::launch_fft_psd<sdr::InF32, true>(const sdr::FftLaunch &, sdr::LaunchAt);
template hipError_t sdr::launch_fft_psd<sdr::InSc16, true>(const sdr::FftLaunch &, sdr::LaunchAt);
