// ddc_shape_probe.cpp — prints sdr::ddc_shape(D, T) of the library's own header (sdrainer_amd/csrc/ddc.h) for the pairs on
// its command line, one line "D T chunk threads width lds_bytes" per pair; with the single argument "grid" and a list of
// tap counts, for every D = 1 .. kDdcMaxDecimation with each of them.  tests/test_ddc_fuzz_coverage.py builds it with g++
// (the header's constexpr arithmetic needs no device compiler) and reads which tile shape a geometry of the fuzz reaches.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../sdrainer_amd/csrc/ddc.h"

static int print_shape(long d, long t)
{
    if (d < 1 || d > sdr::kDdcMaxDecimation || t < 1 || t > sdr::kDdcMaxTaps) {
        std::fprintf(stderr, "ddc_shape_probe: (%ld, %ld) is outside D = 1 .. %d, T = 1 .. %d\n", d, t, sdr::kDdcMaxDecimation, sdr::kDdcMaxTaps);
        return 1;
    }
    const sdr::DdcShape s = sdr::ddc_shape((int)d, (int)t);
    std::printf("%ld %ld %d %d %d %u\n", d, t, s.chunk, s.threads, s.width, s.lds_bytes);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc >= 3 && std::strcmp(argv[1], "grid") == 0) {
        for (long d = 1; d <= sdr::kDdcMaxDecimation; d++)
            for (int i = 2; i < argc; i++)
                if (print_shape(d, std::strtol(argv[i], nullptr, 10)))
                    return 1;
        return 0;
    }
    if (argc < 3 || argc % 2 != 1) {
        std::fprintf(stderr, "usage: ddc_shape_probe D T [D T ...] | ddc_shape_probe grid T [T ...]\n");
        return 2;
    }
    for (int i = 1; i + 1 < argc; i += 2)
        if (print_shape(std::strtol(argv[i], nullptr, 10), std::strtol(argv[i + 1], nullptr, 10)))
            return 1;
    return 0;
}
