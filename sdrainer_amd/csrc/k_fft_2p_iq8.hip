// k_fft_2p_iq8.hip — phase A of the two-phase FFT (N = 32768 / 65536) reading 8-bit frames (cs8 / cu8, iq8.h), plain and
// windowed: k_fft_2p.hip compiled again for k_fft_2p_a.h's 8-bit instances, in a translation unit of its own so that
// k_fft_2p.hip's kernels stay what they were (see that file's header).  Phase B is that unit's.
#define SDR_FFT2P_IQ8 1
#include "k_fft_2p.hip"
