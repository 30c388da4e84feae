// k_fft_r32_iq8.hip — k_fft_r32 reading 8-bit frames (cs8 / cu8, iq8.h): k_fft_r32.hip compiled again, in a translation
// unit of its own so that the other kernels' code stays exactly what it was (see that file's header).
#define SDR_R32_IQ8 1
#include "k_fft_r32.hip"
