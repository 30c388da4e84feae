// Which FFT kernel the batch plan picks (sdrainer_amd/csrc/host/batch_plan.h fft_choice, with the switches the environment
// sets, as a bank reads them): prints "r32 <0|1> wide_tap <0|1> two_phase <0|1>" for the geometry on the command line - the
// kernel family, which does not depend on the input format (tests/test_iq8_gpu.py asserts which family its batches reach).
// With the format and the hop given as well it also prints " kernel <name> id <FftKernel> frames_per_wg <k>": the kernel the
// batch launches first (fft_kernel, fft_kernel_name; tests/test_fft_dispatch_gpu.py).  No GPU, no HIP.
// usage: iq8_plan <n> <frames> <bands> <listener slots> <windowed 0|1> [<format f32|sc16|cs8|cu8> <hop, 0 = dense>]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../sdrainer_amd/csrc/host/batch_plan.h"

int main(int argc, char **argv)
{
    if (argc != 6 && argc != 8) {
        std::fprintf(stderr, "usage: %s <n> <frames> <bands> <slots> <windowed> [<format> <hop>]\n", argv[0]);
        return 2;
    }
    sdr::InFormat fmt = sdr::InFormat::F32;
    if (argc == 8) {
        static const char *const names[] = {"f32", "sc16", "cs8", "cu8"};
        int f = 0;
        while (f < 4 && std::strcmp(argv[6], names[f]) != 0)
            f++;
        if (f == 4) {
            std::fprintf(stderr, "%s: no such format\n", argv[6]);
            return 2;
        }
        fmt = (sdr::InFormat)f;
    }
    const sdr::FftChoice c = sdr::fft_choice(sdr::read_switches(), std::atoi(argv[1]), std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]),
                                             std::atoi(argv[5]) != 0, fmt, argc == 8 ? std::atoi(argv[7]) : 0);
    std::printf("r32 %d wide_tap %d two_phase %d", c.r32 ? 1 : 0, c.wide_tap ? 1 : 0, c.two_phase ? 1 : 0);
    if (argc == 8)
        std::printf(" kernel %s id %d frames_per_wg %d", sdr::fft_kernel_name(sdr::fft_kernel(c)), (int)sdr::fft_kernel(c), c.frames_per_wg);
    std::printf("\n");
    return 0;
}
