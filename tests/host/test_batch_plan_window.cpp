// Host-only test of the batch plan for a bank with a window (sdr_set_window; sdrainer_amd/csrc/host/batch_plan.h): k_fft_r32
// has no windowed form, so windowed N = 16384 is never planned onto it and never gets the wide tap - at any batch length,
// with SDR_FFT_R32 forced on, off or unset - and nothing else about the plan changes; without a window every choice is the
// one it was, at the boundaries tests/host/test_batch_plan.cpp pins.  Built by tests/test_window_host.py.  No GPU, no HIP.
#include <cstdio>
#include <initializer_list>

#include "../../sdrainer_amd/csrc/host/batch_plan.h"

namespace {

int g_failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            g_failures++;                                                        \
        }                                                                        \
    } while (0)

constexpr int C = SDR_CUMULATION_SIZE;

sdr::BatchPlan plan(const sdr::Switches &sw, int bands, int n, int frames, int slots, bool windowed)
{
    const int max_frames = frames > 2048 ? frames : 2048;
    return sdr::plan_batch(sw, sdr::BatchGeometry{bands, n, max_frames, max_frames / C + 2}, frames, 0, false, slots, windowed);
}

bool same_but_fft(const sdr::BatchPlan &a, const sdr::BatchPlan &b)
{
    for (int k = 0; k < sdr::K_COUNT; k++)
        if (a.stream[k] != b.stream[k])
            return false;
    return a.noise_scan == b.noise_scan && a.force_exact == b.force_exact && a.var_mfma == b.var_mfma && a.wm_wpb == b.wm_wpb &&
           a.bound == b.bound && a.bound_done == b.bound_done && a.scan_parts == b.scan_parts && a.n_slots == b.n_slots &&
           a.n_chunks == b.n_chunks && a.new_count == b.new_count && a.refine == b.refine && a.fft.fpw == b.fft.fpw &&
           a.fft.two_phase == b.fft.two_phase && a.fft.group_frames == b.fft.group_frames;
}

}  // namespace

int main()
{
    // windowed N = 16384: never k_fft_r32, never the wide tap
    for (int forced : {-1, 0, 1}) {
        sdr::Switches sw;
        sw.fft_r32 = forced;
        for (int frames : {1, 1023, 1024, 2048, 8192})
            for (int bands : {1, 8})
                for (int slots : {0, 16, 256, 512, 513}) {
                    const sdr::FftChoice c = sdr::fft_choice(sw, 16384, frames, bands, slots, true);
                    CHECK(!c.r32 && !c.wide_tap && !c.two_phase);
                    const sdr::BatchPlan p = plan(sw, bands, 16384, frames, slots, true);
                    CHECK(!p.fft.r32 && !p.fft.wide_tap && !p.fft.two_phase && p.fft.group_frames == 0);
                    // everything but the FFT kernel is planned as without a window
                    CHECK(same_but_fft(p, plan(sw, bands, 16384, frames, slots, false)));
                }
    }
    // the frames-per-workgroup switch still reaches the 16-point kernel
    {
        sdr::Switches sw;
        sw.fft_fpw = 4;
        sw.fft_r32 = 1;
        const sdr::FftChoice c = sdr::fft_choice(sw, 16384, 2048, 1, 16, true);
        CHECK(!c.r32 && c.fpw == 4);
    }
    // the other sizes have one kernel family each: the window changes nothing in the plan
    for (int n : {512, 1024, 2048, 4096, 8192, 32768, 65536})
        for (int frames : {1, 100, 2048}) {
            const sdr::BatchPlan w = plan(sdr::Switches(), 1, n, frames, 16, true), u = plan(sdr::Switches(), 1, n, frames, 16, false);
            CHECK(same_but_fft(w, u) && w.fft.r32 == u.fft.r32 && w.fft.wide_tap == u.fft.wide_tap && !w.fft.r32 && !w.fft.wide_tap);
            CHECK(w.fft.two_phase == (n > 16384));
        }
    // without a window (the default argument and an explicit false): the choices test_batch_plan.cpp pins, at their boundaries
    {
        const sdr::Switches def;
        CHECK(!sdr::fft_choice(def, 16384, 1023, 1, 256).r32 && sdr::fft_choice(def, 16384, 1024, 1, 256).r32);
        CHECK(!sdr::fft_choice(def, 16384, 1023, 1, 256, false).r32 && sdr::fft_choice(def, 16384, 1024, 1, 256, false).r32);
        CHECK(sdr::fft_choice(def, 16384, 128, 8, 16).r32 && !sdr::fft_choice(def, 16384, 127, 8, 16).r32);
        CHECK(sdr::fft_choice(def, 16384, 2048, 1, 512).r32 && !sdr::fft_choice(def, 16384, 2048, 1, 513).r32);
        CHECK(sdr::fft_choice(def, 16384, 2048, 1, 256).wide_tap && !sdr::fft_choice(def, 16384, 2048, 1, 0).wide_tap);
        CHECK(!sdr::fft_choice(def, 8192, 8192, 8, 16).r32);
        sdr::Switches on, off;
        on.fft_r32 = 1;
        off.fft_r32 = 0;
        CHECK(sdr::fft_choice(on, 16384, 1, 1, 16).r32 && sdr::fft_choice(on, 16384, 1, 1, 16).wide_tap);
        CHECK(!sdr::fft_choice(off, 16384, 8192, 1, 16).r32 && !sdr::fft_choice(off, 16384, 8192, 1, 16).wide_tap);
        CHECK(!sdr::fft_choice(on, 16384, 8192, 1, 513).r32);
        const sdr::BatchPlan p = plan(def, 1, 16384, 2048, 256, false);
        CHECK(p.fft.r32 && p.fft.wide_tap);
    }
    std::printf(g_failures ? "FAILED %d\n" : "plan ok\n", g_failures);
    return g_failures ? 1 : 0;
}
