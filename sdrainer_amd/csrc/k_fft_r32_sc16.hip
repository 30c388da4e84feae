// k_fft_r32_sc16.hip — k_fft_r32 for sc16 input (complex int16, sc16.h): k_fft_r32.hip compiled a second time, in a
// translation unit of its own so that the float32 kernel's stays exactly what it was (see that file's header).
#define SDR_R32_SC16 1
#include "k_fft_r32.hip"
