// The cases of DESIGN 3, "Inf / NaN inputs", shared by emu_fft.cpp, emu_fft_r32.cpp and emu_fft_2p.cpp: a frame of noise
// and a tone with ONE sample component replaced by +Inf, -Inf or NaN, in re or in im, at sample 0, N/4, N/2, 3N/4 and an
// odd index.  `kernel` and `oracle` fill the psd row of a frame (any bin order); printed per case is the class of every
// word on both sides:
//   nonfinite N=<n> <value> <re|im> @<index>: kernel <finite> <inf> <nan> oracle <finite> <inf> <nan>
// TEST ONLY, as the drivers that include it.
#pragma once
#include <cmath>
#include <cstdio>
#include <limits>
#include <random>
#include <vector>

struct PsdClasses {
    long finite = 0, inf = 0, nan = 0;
};

static inline PsdClasses classes_of(const std::vector<float> &psd)
{
    PsdClasses c;
    for (float p : psd)
        (std::isnan(p) ? c.nan : std::isinf(p) ? c.inf : c.finite)++;
    return c;
}

template <class K, class O>
static int nonfinite_cases(int n, K kernel, O oracle)
{
    std::mt19937 rng(4242u + (unsigned)n);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> base(2 * (size_t)n);
    for (int i = 0; i < n; i++) {
        base[2 * i] = nd(rng) + 100.f * (float)std::cos(2 * M_PI * 37.0 * i / n);
        base[2 * i + 1] = nd(rng) + 100.f * (float)std::sin(2 * M_PI * 37.0 * i / n);
    }
    const float inf = std::numeric_limits<float>::infinity();
    const struct { const char *name; float v; } values[] = {{"+inf", inf}, {"-inf", -inf}, {"nan", std::nanf("")}};
    const int at[] = {0, n / 4, n / 2, 3 * n / 4, n / 4 + 37};
    std::vector<float> got((size_t)n), want((size_t)n);
    for (const auto &val : values)
        for (int part = 0; part < 2; part++)
            for (int i : at) {
                std::vector<float> iq = base;
                iq[2 * (size_t)i + part] = val.v;
                if (kernel(iq, got) || oracle(iq, want))
                    return 1;
                const PsdClasses k = classes_of(got), o = classes_of(want);
                printf("nonfinite N=%d %s %s @%d: kernel %ld %ld %ld oracle %ld %ld %ld\n", n, val.name, part ? "im" : "re", i,
                       k.finite, k.inf, k.nan, o.finite, o.inf, o.nan);
            }
    return 0;
}
