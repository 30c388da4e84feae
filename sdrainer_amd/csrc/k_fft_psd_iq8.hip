// k_fft_psd_iq8.hip — k_fft_psd for 8-bit input (cs8 / cu8, iq8.h), plain and windowed: k_fft_psd.hip compiled a third
// time, in a translation unit of its own beside the float32 and sc16 kernels' (see that file's header).  Holds k_fft_psd_iq8<9..14, false / true> and launch_fft_psd_iq8 only.
#define SDR_FFT_IQ8 1
#include "k_fft_psd.hip"
