// The sc16 input path's host-checkable parts (sdrainer_amd/csrc/sc16.h), compiled with g++ -ffp-contract=off like the
// library's device code:
//   * the conversion against a correctly rounded division (float64 quotient, rounded once) for all 65 536 inputs;
//   * k_fft_psd_sc16's staging image for N = 512 ... 16384: a bijection of the frame onto N*4 bytes, every DMA row reads
//     exactly its own 1 KB of the frame, every register slot of every thread reads the sample pass 0 wants there, and
//     each 32-lane group of a ds_read_b32 touches 32 different banks (audit_image.h).
// Prints "multiply-wrong: <values>" (the inputs where x * (1/32767) differs, for the GPU test's input) and "ok".
#include <cstdio>
#include <cstring>

#include "../../sdrainer_amd/csrc/sc16.h"
#include "audit_image.h"

static unsigned bits(float f)
{
    unsigned u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main()
{
    int wrong = 0;
    std::printf("multiply-wrong:");
    for (int v = -32768; v <= 32767; v++) {
        const float want = (float)((double)v / 32767.0);  // the double quotient is exact enough to round once
        const float got = sc16::to_f32((int16_t)v);
        if (bits(got) != bits(want)) {
            if (wrong++ < 8)
                std::fprintf(stderr, "to_f32(%d) = %a, want %a\n", v, got, want);
        }
        volatile float inv = 1.0f / 32767.0f;
        if (bits((float)v * inv) != bits(want))
            std::printf(" %d", v);
    }
    std::printf("\n");
    if (wrong) {
        std::printf("conversion wrong for %d inputs\n", wrong);
        return 1;
    }
    // the word helpers: I in the low half, Q in the high half
    if (bits(sc16::re_of(0x80017fffu)) != bits(1.0f) || bits(sc16::im_of(0x80017fffu)) != bits((float)(-32767.0 / 32767.0)))
        return 1;
    // (the float32 image follows the same rule, fft64::PairedSwz: audited here beside tests/emu/emu_fft.cpp's replay)
    if (audit_images<sc16::Image>() | audit_images<fft64::InImageF32>())
        return 1;
    std::printf("ok\n");
    return 0;
}
