// Which FFT kernel the batch plan picks (sdrainer_amd/csrc/host/batch_plan.h fft_choice, with the switches the environment
// sets, as a bank reads them): prints "r32 <0|1> wide_tap <0|1> two_phase <0|1>" for the geometry on the command line.  The
// plan does not look at the input format, so this is the kernel family an 8-bit batch of that geometry runs
// (tests/test_iq8_gpu.py asserts which of k_fft_r32_iq8 and k_fft_psd_iq8<14> its batches reach).  No GPU, no HIP.
// usage: iq8_plan <n> <frames> <bands> <listener slots> <windowed 0|1>
#include <cstdio>
#include <cstdlib>

#include "../../sdrainer_amd/csrc/host/batch_plan.h"

int main(int argc, char **argv)
{
    if (argc != 6) {
        std::fprintf(stderr, "usage: %s <n> <frames> <bands> <slots> <windowed>\n", argv[0]);
        return 2;
    }
    const sdr::FftChoice c = sdr::fft_choice(sdr::read_switches(), std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]),
                                             std::atoi(argv[5]) != 0);
    std::printf("r32 %d wide_tap %d two_phase %d\n", c.r32 ? 1 : 0, c.wide_tap ? 1 : 0, c.two_phase ? 1 : 0);
    return 0;
}
