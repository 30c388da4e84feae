// Emulates k_fft_2p.hip's two phases thread by thread on the CPU, with the very index and butterfly functions the kernels
// compile (sdrainer_amd/csrc/fft_2p.h): every workgroup's threads load, run pass 0, write the exchange area, then (behind
// the barrier) read it back, run pass 1 and store - phase A into the float64 intermediate, phase B into the fft-shifted
// psd row and the listener tap.  Compared bit for bit with the oracle's stage-by-stage radix-2 FFT and PSD
// (oracle/sdr_oracle.c: orc_iq_to_spectrum_and_psd), at N = 32768 and 65536, float32 and sc16 input (the latter through
// sc16.h's conversion, as the kernel reads it), random, full-scale and zero frames.
//   usage: emu_fft_2p <liborc.so>        prints "<case>: <k> mismatches" per case
//          emu_fft_2p <liborc.so> nonfinite     the psd classes of frames with one non-finite sample (nonfinite_classes.h)
#include <dlfcn.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../sdrainer_amd/csrc/fft_2p.h"
#include "../../sdrainer_amd/csrc/twiddles.h"
#include "nonfinite_classes.h"

typedef void (*orc_psd_t)(int, const float *, float *, float *);

using fft64::cplx;

template <int LOGN>
struct Emu {
    using PH = fft2p::Phases<LOGN>;
    static constexpr int N = PH::N, A = PH::A, B = PH::B;
    std::vector<cplx> tw;
    Emu()
    {
        std::vector<double> re, im;
        fft64::radix2_factors(N, re, im);
        tw.resize(N / 2);
        for (int i = 0; i < N / 2; i++)
            tw[i] = cplx{re[i], im[i]};
    }
    cplx W(int i) const
    {
        if (i < 0 || i >= N / 2) {
            fprintf(stderr, "twiddle index %d out of range\n", i);
            exit(2);
        }
        return tw[i];
    }
    // phase A of one frame; `x(i)` returns sample i as the kernel converts it
    template <class X>
    void phase_a(X x, std::vector<cplx> &y) const
    {
        using S = typename PH::SA;
        constexpr int MB = A;
        auto Wf = [this](int i) { return W(i); };
        std::vector<double> lr(S::G * S::LDS_ROW), li(S::G * S::LDS_ROW);
        static double xr[fft2p::T][fft2p::R], xi[fft2p::T][fft2p::R];
        for (int w = 0; w < PH::WG_A; w++) {
            for (int t = 0; t < fft2p::T; t++) {
                const int gl = fft2p::p0_sub<MB>(t), p = w * S::G + gl;
                for (int s = 0; s < fft2p::R; s++) {
                    const int i = fft2p::a_sample<LOGN>(p, fft2p::p0_index<MB>(t, s));
                    x(i, xr[t][s], xi[t][s]);
                }
                fft2p::pass0<MB>(xr[t], xi[t], LOGN, 0, 0, t, Wf);
                for (int s = 0; s < fft2p::R; s++) {
                    const int at = gl * S::LDS_ROW + fft2p::p0_index<MB>(t, s);
                    lr[at] = xr[t][s];
                    li[at] = xi[t][s];
                }
            }
            for (int t = 0; t < fft2p::T; t++) {
                const int gl = fft2p::p1_sub<MB, true>(t);
                for (int s = 0; s < fft2p::R; s++) {
                    const int at = gl * S::LDS_ROW + fft2p::p1_index<MB, true>(t, s);
                    xr[t][s] = lr[at];
                    xi[t][s] = li[at];
                }
                fft2p::pass1<MB, true>(xr[t], xi[t], LOGN, 0, 0, t, Wf);
                const int k = fft2p::a_block<LOGN>(w * S::G + gl);
                for (int s = 0; s < fft2p::R; s++)
                    y[((size_t)k << A) + fft2p::p1_index<MB, true>(t, s)] = cplx{xr[t][s], xi[t][s]};
            }
        }
    }
    void phase_b(const std::vector<cplx> &y, std::vector<float> &psd, const std::vector<int> &bins, std::vector<float> &tap) const
    {
        using S = typename PH::SB;
        constexpr int MB = B;
        auto Wf = [this](int i) { return W(i); };
        std::vector<double> lr(S::G * S::LDS_ROW), li(S::G * S::LDS_ROW);
        std::vector<float> prow(S::G << MB);
        static double xr[fft2p::T][fft2p::R], xi[fft2p::T][fft2p::R];
        for (int w = 0; w < PH::WG_B; w++) {
            const int c0 = w * S::G;
            for (int t = 0; t < fft2p::T; t++) {
                const int gl = fft2p::p0_sub<MB>(t), c = c0 + gl;
                for (int s = 0; s < fft2p::R; s++) {
                    const cplx v = y[c + ((size_t)fft2p::p0_index<MB>(t, s) << A)];
                    xr[t][s] = v.x;
                    xi[t][s] = v.y;
                }
                fft2p::pass0<MB>(xr[t], xi[t], LOGN, A, c, t, Wf);
                for (int s = 0; s < fft2p::R; s++) {
                    const int at = gl * S::LDS_ROW + fft2p::p0_index<MB>(t, s);
                    lr[at] = xr[t][s];
                    li[at] = xi[t][s];
                }
            }
            for (int t = 0; t < fft2p::T; t++) {
                const int gl = fft2p::p1_sub<MB, false>(t), c = c0 + gl;
                for (int s = 0; s < fft2p::R; s++) {
                    const int at = gl * S::LDS_ROW + fft2p::p1_index<MB, false>(t, s);
                    xr[t][s] = lr[at];
                    xi[t][s] = li[at];
                }
                fft2p::pass1<MB, false>(xr[t], xi[t], LOGN, A, c, t, Wf);
                for (int s = 0; s < fft2p::R; s++) {
                    const float p = fft2p::psd_of(xr[t][s], xi[t][s]);
                    psd[(c + (fft2p::p1_index<MB, false>(t, s) << A)) ^ (N / 2)] = p;
                    prow[gl * (1 << MB) + fft2p::p1_index<MB, false>(t, s)] = p;
                }
            }
            for (int l = 0; l < (int)bins.size(); l++) {
                const int bin = bins[l];
                if (bin < 0) {
                    if (w == 0)
                        tap[l] = 0.0f;
                    continue;
                }
                const int idx = bin ^ (N / 2), cl = (idx & ((1 << A) - 1)) - c0;
                if (cl >= 0 && cl < S::G)
                    tap[l] = prow[cl * (1 << MB) + (idx >> A)];
            }
        }
    }
};

template <int LOGN>
static int run(orc_psd_t orc, const char *kind, bool sc16in, unsigned seed)
{
    Emu<LOGN> emu;
    constexpr int N = 1 << LOGN;
    std::mt19937 rng(seed);
    std::vector<float> iq(2 * N), spec(N), want(N), psd(N, -1.0f);
    std::vector<uint32_t> words(N);
    std::vector<cplx> y(N);
    std::uniform_int_distribution<int> d16(-32768, 32767);
    std::normal_distribution<float> nd(0.0f, 0.3f);
    for (int i = 0; i < N; i++) {
        int16_t re = 0, im = 0;
        if (!strcmp(kind, "random")) {
            re = (int16_t)d16(rng);
            im = (int16_t)d16(rng);
        } else if (!strcmp(kind, "fullscale")) {
            re = (i & 1) ? -32768 : 32767;
            im = (i & 2) ? 32767 : -32768;
        }
        words[i] = (uint32_t)(uint16_t)re | (uint32_t)(uint16_t)im << 16;
        if (sc16in) {
            iq[2 * i] = sc16::re_of(words[i]);
            iq[2 * i + 1] = sc16::im_of(words[i]);
        } else if (!strcmp(kind, "random")) {
            iq[2 * i] = nd(rng) + 0.2f * std::cos(0.01f * i);
            iq[2 * i + 1] = nd(rng);
        } else if (!strcmp(kind, "fullscale")) {
            iq[2 * i] = (i & 1) ? -1.0f : 1.0f;
            iq[2 * i + 1] = 1e30f * ((i & 2) ? 1.0f : -1.0f);
        } else {
            iq[2 * i] = iq[2 * i + 1] = 0.0f;
        }
    }
    if (sc16in)
        emu.phase_a([&](int i, double &re, double &im) { re = (double)sc16::re_of(words[i]); im = (double)sc16::im_of(words[i]); }, y);
    else
        emu.phase_a([&](int i, double &re, double &im) { re = (double)iq[2 * i]; im = (double)iq[2 * i + 1]; }, y);
    // listeners: random bins, a free slot, the edges of the row
    std::vector<int> bins = {0, N - 1, N / 2, N / 2 - 1, -1, 1, 12345 % N};
    for (int l = 0; l < 249; l++)
        bins.push_back((int)(rng() % N));
    std::vector<float> tap(bins.size(), -7.0f);
    emu.phase_b(y, psd, bins, tap);
    orc(N, iq.data(), spec.data(), want.data());
    long bad = 0;
    for (int k = 0; k < N; k++)
        bad += memcmp(&psd[k], &want[k], 4) != 0;
    long tap_bad = 0;
    for (size_t l = 0; l < bins.size(); l++) {
        const float w = bins[l] < 0 ? 0.0f : want[bins[l]];
        tap_bad += memcmp(&tap[l], &w, 4) != 0;
    }
    printf("N=%d %s %s: %ld mismatches, tap %ld mismatches\n", N, sc16in ? "sc16" : "f32", kind, bad, tap_bad);
    return bad || tap_bad;
}

// the psd classes of frames with one non-finite sample component, both phases and oracle (nonfinite_classes.h)
template <int LOGN>
static int nonfinite(orc_psd_t orc)
{
    Emu<LOGN> emu;
    constexpr int N = 1 << LOGN;
    return nonfinite_cases(N, [&](const std::vector<float> &iq, std::vector<float> &psd) {
        std::vector<cplx> y(N);
        std::vector<int> bins;
        std::vector<float> tap;
        emu.phase_a([&](int i, double &re, double &im) { re = (double)iq[2 * i]; im = (double)iq[2 * i + 1]; }, y);
        emu.phase_b(y, psd, bins, tap);
        return 0;
    }, [&](const std::vector<float> &iq, std::vector<float> &psd) {
        std::vector<float> spec(N);
        orc(N, iq.data(), spec.data(), psd.data());
        return 0;
    });
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: %s liborc.so\n", argv[0]);
        return 2;
    }
    void *h = dlopen(argv[1], RTLD_NOW);
    if (!h) {
        fprintf(stderr, "dlopen: %s\n", dlerror());
        return 2;
    }
    auto orc = (orc_psd_t)dlsym(h, "orc_iq_to_spectrum_and_psd");
    if (!orc)
        return 2;
    if (argc > 2 && !strcmp(argv[2], "nonfinite"))
        return nonfinite<15>(orc) | nonfinite<16>(orc);
    int rc = 0;
    for (const char *kind : {"random", "fullscale", "zero"})
        for (bool s : {false, true}) {
            rc |= run<15>(orc, kind, s, 15u + (unsigned)s);
            rc |= run<16>(orc, kind, s, 16u + (unsigned)s);
        }
    return rc;
}
