// k_fft_r32_hop_sc16.hip — k_fft_r32_sc16 for overlapped frames: k_fft_r32.hip compiled once more (see that file's header).
#define SDR_R32_HOP 1
#define SDR_R32_SC16 1
#include "k_fft_r32.hip"
