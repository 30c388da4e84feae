// k_fft_psd_win.hip — k_fft_psd and k_fft_psd_sc16 with a window on the frames (sdr_set_window): k_fft_psd.hip compiled
// again, in a translation unit of its own so that the plain kernels' code stays exactly what it was (see that file's
// header).
#define SDR_FFT_WIN 1
#include "k_fft_psd.hip"
