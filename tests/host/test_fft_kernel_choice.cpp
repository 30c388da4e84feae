// Host-only test of which FFT kernel a batch reaches (sdrainer_amd/csrc/host/batch_plan.h: fft_choice -> fft_kernel ->
// fft_kernel_name).  The expectation is the launchers' hand-on chain as it stood before the plan named the kernel -
// launch_fft -> launch_fft_2p(_iq8) / launch_fft_iq8 / launch_fft_r32*(_hop*) / launch_fft_win / launch_fft_t - written
// out arm by arm below, not computed by the functions under test; the switches go through the environment and
// read_switches(), as a bank reads them.  Built by tests/test_fft_kernel_choice.py.  No GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../sdrainer_amd/csrc/host/batch_plan.h"

namespace {

using sdr::FftKernel;
using sdr::InFormat;

int g_failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            g_failures++;                                                        \
        }                                                                        \
    } while (0)

struct Case {
    int n, frames, bands, slots, hop;  // hop: 0 = dense
    InFormat fmt;
    bool windowed;
    int env_r32, env_fpw;  // SDR_FFT_R32 / SDR_FFT_FPW as set in the environment (-1 / 0: unset)
};

// fft_choice's rule for k_fft_r32 as it has stood since the window PR
bool old_r32(const Case &c)
{
    if (c.windowed || c.n != 16384 || c.slots > 512)
        return false;
    if (c.env_r32 >= 0)
        return c.env_r32 != 0;
    return (long)c.frames * c.bands >= 1024;
}

// launch_fft_t's frames per workgroup: kDefaultFpw = 1, halved while fewer than 256 workgroups would remain
int old_fpw(const Case &c)
{
    int fpw = c.env_fpw > 0 ? c.env_fpw : 1;
    while (fpw > 1 && (long)((c.frames + fpw - 1) / fpw) * c.bands < 256)
        fpw /= 2;
    return fpw;
}

// the kernel the old chain launched first; *refused: one of its run-time refusals was reached
FftKernel old_chain(const Case &c, bool *refused)
{
    using K = FftKernel;
    const bool r32 = old_r32(c), two_phase = c.n > 16384, window = c.windowed;
    const int frame_stride = c.hop ? c.hop : c.n;
    *refused = false;
    if (two_phase) {  // launch_fft -> launch_fft_2p
        if (sdr::is_iq8(c.fmt)) {  // -> launch_fft_2p_iq8: launch_fft2p_iq8_t<LOGN, CS8 / CU8>
            if (c.fmt == InFormat::CU8)
                return window ? K::A2P_WIN_CU8 : K::A2P_CU8;
            return window ? K::A2P_WIN_CS8 : K::A2P_CS8;
        }
        // launch_fft2p_t
        if (window && c.fmt == InFormat::SC16)
            return K::A2P_WIN_SC16;
        if (window)
            return K::A2P_WIN_F32;
        if (c.fmt == InFormat::SC16)
            return K::A2P_SC16;
        return K::A2P_F32;
    }
    if (sdr::is_iq8(c.fmt)) {
        if (!r32)  // -> launch_fft_iq8: k_fft_psd_iq8<LOGN, true / false> by tap.window
            return window ? K::PSD_IQ8_WIN : K::PSD_IQ8;
        if (c.n != 16384 || window)
            *refused = true;
        // -> launch_fft_r32_iq8, which handed frame_stride != N on to launch_fft_r32_hop_iq8
        return frame_stride != c.n ? K::R32_HOP_IQ8 : K::R32_IQ8;
    }
    if (window) {  // -> launch_fft_win -> the windowed unit's launch_fft_t
        if (r32 || two_phase)
            *refused = true;
        if (c.fmt == InFormat::SC16)
            return K::PSD_SC16_WIN;
        return old_fpw(c) > 1 ? K::PSD_WIN_MULTI : K::PSD_WIN;
    }
    if (r32) {
        if (c.n != 16384)
            *refused = true;
        if (c.fmt == InFormat::SC16)  // -> launch_fft_r32_sc16 (-> launch_fft_r32_hop_sc16)
            return frame_stride != c.n ? K::R32_HOP_SC16 : K::R32_SC16;
        return frame_stride != c.n ? K::R32_HOP : K::R32;  // -> launch_fft_r32 (-> launch_fft_r32_hop)
    }
    // launch_fft_t
    if (c.fmt == InFormat::SC16)
        return K::PSD_SC16;
    return old_fpw(c) > 1 ? K::PSD_MULTI : K::PSD;
}

// the kernels' labels: the base names their symbols had when each kernel was a function of its own, as
// profiles/*_kernel_resources.txt spell them (today k_fft_psd.h, k_fft_r32.h and k_fft_2p_a.h hold templates; the labels stay)
const char *old_name(FftKernel k)
{
    static const char *const names[(int)FftKernel::COUNT] = {
        "k_fft_psd",     "k_fft_psd",      "k_fft_psd_sc16", "k_fft_psd_iq8", "k_fft_psd_win",      "k_fft_psd_win",
        "k_fft_psd_sc16_win", "k_fft_psd_iq8", "k_fft_r32",  "k_fft_r32_sc16", "k_fft_r32_iq8",     "k_fft_r32_hop",
        "k_fft_r32_hop_sc16", "k_fft_r32_hop_iq8", "k_fft2p_a", "k_fft2p_a",  "k_fft2p_a",          "k_fft2p_a",
        "k_fft2p_win_a", "k_fft2p_win_a",  "k_fft2p_win_a",  "k_fft2p_win_a"};
    return names[(int)k];
}

void set_env(const char *name, int value, int unset)
{
    if (value == unset) {
        unsetenv(name);
        return;
    }
    char buf[16];
    std::snprintf(buf, sizeof buf, "%d", value);
    setenv(name, buf, 1);
}

sdr::FftChoice choose(const Case &c)
{
    set_env("SDR_FFT_R32", c.env_r32, -1);
    set_env("SDR_FFT_FPW", c.env_fpw, 0);
    return sdr::fft_choice(sdr::read_switches(), c.n, c.frames, c.bands, c.slots, c.windowed, c.fmt, c.hop);
}

// what a launcher instance checks before it launches (k_fft_psd.h, k_fft_r32.h, k_fft_2p_a.h): none may refuse a planned choice
bool a_unit_takes(const sdr::FftChoice &c, int n, int slots, int frame_stride)
{
    switch (sdr::fft_kernel(c)) {
    case FftKernel::R32: case FftKernel::R32_SC16: case FftKernel::R32_IQ8:
        return n == 16384 && !c.windowed && slots <= 512 && frame_stride == n;
    case FftKernel::R32_HOP: case FftKernel::R32_HOP_SC16: case FftKernel::R32_HOP_IQ8:
        return n == 16384 && !c.windowed && slots <= 512 && frame_stride < n && (frame_stride & (frame_stride - 1)) == 0;
    case FftKernel::A2P_F32: case FftKernel::A2P_SC16: case FftKernel::A2P_CS8: case FftKernel::A2P_CU8:
    case FftKernel::A2P_WIN_F32: case FftKernel::A2P_WIN_SC16: case FftKernel::A2P_WIN_CS8: case FftKernel::A2P_WIN_CU8:
        return n == 32768 || n == 65536;
    case FftKernel::PSD_MULTI: case FftKernel::PSD_WIN_MULTI:
        return n >= 512 && n <= 16384 && c.fmt == InFormat::F32 && c.frames_per_wg > 1;
    case FftKernel::COUNT:
        return false;
    default:
        return n >= 512 && n <= 16384 && c.frames_per_wg == 1;
    }
}

}  // namespace

int main()
{
    // the full product: the kernel and its name
    bool reached[(int)FftKernel::COUNT] = {};
    for (int n : {512, 8192, 16384, 32768, 65536})
        for (InFormat fmt : {InFormat::F32, InFormat::SC16, InFormat::CS8, InFormat::CU8})
            for (bool windowed : {false, true})
                for (int hop : {0, n / 4})
                    for (int frames : {1023, 1024})
                        for (int slots : {0, 512, 513})
                            for (int env_r32 : {-1, 0, 1})
                                for (int env_fpw : {0, 2, 4, 64}) {
                                    const Case c{n, frames, 1, slots, hop, fmt, windowed, env_r32, env_fpw};
                                    bool refused;
                                    const FftKernel want = old_chain(c, &refused);
                                    const sdr::FftChoice got = choose(c);
                                    const FftKernel k = sdr::fft_kernel(got);
                                    CHECK(!refused);  // no planned batch ever reached one of the launchers' refusals
                                    CHECK(k == want);
                                    CHECK(std::strcmp(sdr::fft_kernel_name(k), old_name(want)) == 0);
                                    CHECK(a_unit_takes(got, n, slots, hop ? hop : n));
                                    // the new fields say what the arguments said; the old ones are the rule's
                                    CHECK(got.fmt == fmt && got.windowed == windowed && got.strided == (hop != 0));
                                    CHECK(got.r32 == old_r32(c) && got.two_phase == (n > 16384) && got.wide_tap == (old_r32(c) && slots > 0));
                                    CHECK(got.fpw == env_fpw);
                                    CHECK(got.frames_per_wg == (got.r32 || got.two_phase ? 0 : fmt != InFormat::F32 ? 1 : old_fpw(c)));
                                    reached[(int)k] = true;
                                }
    for (int k = 0; k < (int)FftKernel::COUNT; k++)
        CHECK(reached[k]);

    // hop = N is dense; several bands count towards the r32 rule as frames x bands
    {
        const Case dense{16384, 1024, 1, 8, 16384, InFormat::F32, false, -1, 0};
        CHECK(!choose(dense).strided && sdr::fft_kernel(choose(dense)) == FftKernel::R32);
        const Case a{16384, 128, 8, 8, 4096, InFormat::CS8, false, -1, 0}, b{16384, 127, 8, 8, 4096, InFormat::CS8, false, -1, 0};
        CHECK(sdr::fft_kernel(choose(a)) == FftKernel::R32_HOP_IQ8 && sdr::fft_kernel(choose(b)) == FftKernel::PSD_IQ8);
    }
    std::printf(g_failures ? "kernels FAILED\n" : "kernels ok\n");

    // frames per workgroup: the halving rule either side of 256 workgroups, one band
    const int before = g_failures;
    {
        struct {
            int fpw, frames, want;
        } rows[] = {{4, 1020, 2}, {4, 1021, 4}, {4, 1024, 4}, {4, 510, 1}, {4, 511, 2},          // 255 / 256 workgroups of 4, of 2
                    {2, 510, 1},  {2, 511, 2},  {2, 512, 2},                                    // ... of 2
                    {64, 16320, 32}, {64, 16321, 64}, {64, 16384, 64}, {64, 255, 1}, {64, 256, 1}, {64, 511, 2},  // ... of 64, and all the way down
                    {0, 100000, 1}, {1, 100000, 1}};                                           // the default is one frame per workgroup
        for (const auto &r : rows)
            for (bool windowed : {false, true}) {
                const Case c{8192, r.frames, 1, 4, 0, InFormat::F32, windowed, -1, r.fpw};
                const sdr::FftChoice got = choose(c);
                CHECK(got.frames_per_wg == r.want);
                CHECK(sdr::fft_kernel(got) == (r.want > 1 ? (windowed ? FftKernel::PSD_WIN_MULTI : FftKernel::PSD_MULTI)
                                                          : (windowed ? FftKernel::PSD_WIN : FftKernel::PSD)));
            }
        // with several bands the workgroups of every band count: 2 bands x 128 workgroups of 4
        CHECK(choose(Case{8192, 512, 2, 4, 0, InFormat::F32, false, -1, 4}).frames_per_wg == 4);
        CHECK(choose(Case{8192, 508, 2, 4, 0, InFormat::F32, false, -1, 4}).frames_per_wg == 2);
        // sc16 and 8-bit input have no multi-frame form; k_fft_r32 and the two-phase kernels no such notion
        for (InFormat fmt : {InFormat::SC16, InFormat::CS8, InFormat::CU8})
            CHECK(choose(Case{8192, 100000, 1, 4, 0, fmt, false, -1, 64}).frames_per_wg == 1);
        CHECK(choose(Case{16384, 100000, 1, 4, 0, InFormat::F32, false, -1, 64}).frames_per_wg == 0);
        CHECK(choose(Case{16384, 100000, 1, 4, 0, InFormat::F32, false, 0, 64}).frames_per_wg == 64);
        CHECK(choose(Case{32768, 100000, 1, 4, 0, InFormat::F32, false, -1, 64}).frames_per_wg == 0);
        CHECK(sdr::kDefaultFpw == 1);
    }
    std::printf(g_failures != before ? "frames_per_wg FAILED\n" : "frames_per_wg ok\n");

    // plan_batch hands the format and the hop through, and changes nothing else by them
    const int before2 = g_failures;
    {
        unsetenv("SDR_FFT_R32");
        unsetenv("SDR_FFT_FPW");
        const sdr::Switches sw = sdr::read_switches();
        const sdr::BatchGeometry g{1, 16384, 2048, 2048 / SDR_CUMULATION_SIZE + 2};
        const sdr::BatchPlan a = sdr::plan_batch(sw, g, 2048, 0, false, 8), b = sdr::plan_batch(sw, g, 2048, 0, false, 8, false, 0, false, InFormat::CU8, 4096);
        CHECK(sdr::fft_kernel(a.fft) == FftKernel::R32 && sdr::fft_kernel(b.fft) == FftKernel::R32_HOP_IQ8);
        CHECK(a.fft.r32 == b.fft.r32 && a.fft.wide_tap == b.fft.wide_tap && a.fft.reserve_cus == b.fft.reserve_cus && a.fft.group_frames == b.fft.group_frames);
        CHECK(a.bound == b.bound && a.scan_parts == b.scan_parts && a.n_slots == b.n_slots && a.refine == b.refine && a.noise_scan == b.noise_scan);
    }
    std::printf(g_failures != before2 ? "plan FAILED\n" : "plan ok\n");
    return g_failures ? 1 : 0;
}
