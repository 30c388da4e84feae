// k_fft_r32_hop.hip — k_fft_r32 for overlapped frames (a frame stride below N): k_fft_r32.hip compiled again, in a
// translation unit of its own so that the dense kernel's stays exactly what it was (see that file's header).
#define SDR_R32_HOP 1
#include "k_fft_r32.hip"
