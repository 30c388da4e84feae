// The 8-bit input path's host-checkable parts (sdrainer_amd/csrc/iq8.h), compiled with g++ -ffp-contract=off like the
// library's device code:
//   * both conversions (cs8, cu8) for all 256 inputs against the exact rationals x / 128 and (2 x - 255) / 256, in
//     float64, exact equality;
//   * k_fft_psd_iq8's staging image for N = 512 ... 16384: a bijection of the frame onto N*2 bytes, every DMA row reads
//     exactly its own 1 KB of the frame, every register slot of every thread reads the sample pass 0 wants there;
//   * the bank audit: the 32 lanes of each half of a wave's 16-bit read touch dwords that are equal or lie in different
//     banks (32 banks of four bytes; the two halves of one dword are served together) - audit_image.h.
// Prints "cs8:" and "cu8:" with the 256 values each (hex floats) and "ok".
#include <cstdio>

#include "../../sdrainer_amd/csrc/iq8.h"
#include "audit_image.h"

int main()
{
    const iq8::Format cs8 = iq8::format_of(false), cu8 = iq8::format_of(true);
    int wrong = 0;
    std::printf("cs8:");
    for (int v = -128; v <= 127; v++) {
        const uint32_t w = (uint32_t)(uint8_t)(int8_t)v;
        // the byte in the I place with another byte beside it, and in the Q place
        const float re = iq8::re_of(w | 0x5a00u, cs8), im = iq8::im_of((w << 8) | 0xa5u, cs8);
        const double want = (double)v / 128.0;
        if ((double)re != want || (double)im != want)
            wrong++;
        std::printf(" %a", re);
    }
    std::printf("\ncu8:");
    for (int v = 0; v <= 255; v++) {
        const uint32_t w = (uint32_t)v;
        const float re = iq8::re_of(w | 0x5a00u, cu8), im = iq8::im_of((w << 8) | 0xa5u, cu8);
        const double want = (2.0 * v - 255.0) / 256.0;
        if ((double)re != want || (double)im != want)
            wrong++;
        std::printf(" %a", re);
    }
    std::printf("\n");
    if (wrong) {
        std::printf("conversion wrong for %d inputs\n", wrong);
        return 1;
    }
    if (audit_images<iq8::Image>())
        return 1;
    std::printf("ok\n");
    return 0;
}
