// k_fft_r32_hop_iq8.hip — k_fft_r32_iq8 for overlapped frames (a frame stride below N): k_fft_r32.hip compiled again, see
// that file's header.
#define SDR_R32_IQ8 1
#define SDR_R32_HOP 1
#include "k_fft_r32.hip"
