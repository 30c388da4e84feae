// Host-only test of the CUs k_fft_r32's grid leaves free (FftChoice::reserve_cus; sdrainer_amd/csrc/host/batch_plan.h
// fft_reserve_cus): the rule on both sides of every boundary it has (a shared hardware queue among them), its clamp, the forced
// switch (SDR_FFT_RESERVE), and
// that a captured batch takes the same rule from its capture-time geometry.  Built by tests/test_batch_plan_reserve.py.
// No GPU, no HIP.
#include <cstdio>
#include <cstdlib>
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

sdr::BatchPlan plan(const sdr::Switches &sw, int bands, int n, int frames, int count0 = 0, bool capturing = false, int slots = 256,
                    bool windowed = false)
{
    const int max_frames = frames > 2048 ? frames : 2048;
    return sdr::plan_batch(sw, sdr::BatchGeometry{bands, n, max_frames, max_frames / C + 2}, frames, count0, capturing, slots, windowed);
}

// the rule, restated: ceil(scan workgroups / rounds) + extra, clamped
int want(const sdr::BatchPlan &p, int bands)
{
    const int wgs = p.n_slots * p.scan_parts * bands;
    const int r = (wgs + sdr::kReserveRounds - 1) / sdr::kReserveRounds + sdr::kReserveExtra;
    return r > sdr::kReserveMax ? sdr::kReserveMax : r;
}

}  // namespace

int main()
{
    const sdr::Switches def;
    static_assert(sdr::kReserveRounds >= 1 && sdr::kReserveRounds <= 2, "the scan gets its CUs in at most two rounds");
    static_assert(sdr::kReserveMax == 64 && sdr::kReserveMinFrames == 2048, "the constants the sweep chose");
    CHECK(def.fft_reserve == -1);

    // config 3 at bench.py's batch lengths: the sweep's winner at 8192 frames (82 or 83 slots), the same at 4096
    for (int count0 : {0, 1, 57, 99}) {
        CHECK(plan(def, 1, 16384, 8192, count0).fft.reserve_cus == 64);
        CHECK(plan(def, 1, 16384, 4096, count0).fft.reserve_cus == 64);
    }
    // 2048 frames: 21 slots in two parts (count0 = 0) -> 42 / 2 + 24; 22 slots when the batch straddles one more cumulation
    CHECK(plan(def, 1, 16384, 2048, 0).n_slots == 21 && plan(def, 1, 16384, 2048, 0).scan_parts == 2);
    CHECK(plan(def, 1, 16384, 2048, 0).fft.reserve_cus == 45);
    CHECK(plan(def, 1, 16384, 2048, 60).n_slots == 22 && plan(def, 1, 16384, 2048, 60).fft.reserve_cus == 46);

    // below and at the smallest batch that reserves (frames x bands), one band and 24 bands
    CHECK(plan(def, 1, 16384, sdr::kReserveMinFrames - 1).fft.r32 && plan(def, 1, 16384, sdr::kReserveMinFrames - 1).fft.reserve_cus == 0);
    CHECK(plan(def, 1, 16384, sdr::kReserveMinFrames).fft.reserve_cus > 0);
    CHECK(plan(def, 1, 16384, 1024).fft.r32 && plan(def, 1, 16384, 1024).fft.reserve_cus == 0);
    CHECK(plan(def, 24, 16384, 85).fft.r32 && plan(def, 24, 16384, 85).fft.reserve_cus == 0);  // 2040 frames in all
    CHECK(plan(def, 24, 16384, 86).fft.reserve_cus == 48);  // 2064 in all: one slot x two parts x 24 bands = 48 workgroups -> 24 + 24
    for (int bands : {1, 24})
        for (int frames : {2048, 2049, 3000, 4096, 8192})
            for (int count0 : {0, 33, 99}) {
                const sdr::BatchPlan p = plan(def, bands, 16384, frames, count0);
                CHECK(p.fft.r32 && p.fft.reserve_cus == want(p, bands));
                CHECK(p.fft.reserve_cus > 0 && p.fft.reserve_cus <= sdr::kReserveMax);
            }

    // the clamp: many scan workgroups never reserve more than kReserveMax
    {
        const sdr::BatchPlan p = plan(def, 24, 16384, 8192);
        CHECK(p.n_slots * p.scan_parts * 24 > 1000 && p.fft.reserve_cus == sdr::kReserveMax);
        const sdr::FftChoice c = sdr::fft_choice(def, 16384, 8192, 1, 256);
        CHECK(sdr::fft_reserve_cus(def, c, true, 8192, 1, 1 << 20) == sdr::kReserveMax);
        CHECK(sdr::fft_reserve_cus(def, c, true, 8192, 1, 2 * (sdr::kReserveMax - sdr::kReserveExtra)) == sdr::kReserveMax);
        CHECK(sdr::fft_reserve_cus(def, c, true, 8192, 1, 2 * (sdr::kReserveMax - sdr::kReserveExtra) - 2) == sdr::kReserveMax - 1);
        CHECK(sdr::fft_reserve_cus(def, c, true, 8192, 1, 0) == sdr::kReserveExtra);
    }

    // noise_scan off (the chains): no reserve
    {
        sdr::Switches chains;
        chains.noise_scan = false;
        for (int frames : {2048, 8192}) {
            const sdr::BatchPlan p = plan(chains, 1, 16384, frames);
            CHECK(p.fft.r32 && !p.noise_scan && p.fft.reserve_cus == 0);
        }
    }
    // batches that do not run k_fft_r32: a windowed bank, N != 16384, too many listener slots, SDR_FFT_R32=0 - forced or not
    for (int forced : {-1, 0, 1, 48, 300}) {
        sdr::Switches sw;
        sw.fft_reserve = forced;
        for (int frames : {2048, 8192}) {
            CHECK(!plan(sw, 1, 16384, frames, 0, false, 256, true).fft.r32 && plan(sw, 1, 16384, frames, 0, false, 256, true).fft.reserve_cus == 0);
            for (int n : {512, 4096, 8192, 32768, 65536})
                for (int bands : {1, 8})
                    CHECK(!plan(sw, bands, n, frames).fft.r32 && plan(sw, bands, n, frames).fft.reserve_cus == 0);
            CHECK(!plan(sw, 1, 16384, frames, 0, false, 513).fft.r32 && plan(sw, 1, 16384, frames, 0, false, 513).fft.reserve_cus == 0);
            sdr::Switches off = sw;
            off.fft_r32 = 0;
            CHECK(!plan(off, 1, 16384, frames).fft.r32 && plan(off, 1, 16384, frames).fft.reserve_cus == 0);
        }
    }

    // the FFT's stream shares a hardware queue with one of the bank's (sdr_bank::fft_queue_alone false): nothing can run beside
    // an FFT launch, so the rule reserves nothing - and changes nothing else in the plan; a forced reserve is still taken
    for (int frames : {2048, 4096, 8192})
        for (int bands : {1, 24}) {
            const int max_frames = frames;
            const sdr::BatchPlan shared = sdr::plan_batch(def, sdr::BatchGeometry{bands, 16384, max_frames, max_frames / C + 2, false}, frames, 0, false, 256);
            const sdr::BatchPlan alone = sdr::plan_batch(def, sdr::BatchGeometry{bands, 16384, max_frames, max_frames / C + 2, true}, frames, 0, false, 256);
            CHECK(shared.fft.r32 && shared.fft.reserve_cus == 0 && !shared.fft.reserve_forced);
            CHECK(alone.fft.reserve_cus > 0 && alone.fft.reserve_cus == plan(def, bands, 16384, frames).fft.reserve_cus);
            CHECK(shared.scan_parts == alone.scan_parts && shared.n_slots == alone.n_slots && shared.refine == alone.refine && shared.bound == alone.bound);
            sdr::Switches sw;
            sw.fft_reserve = 48;
            const sdr::BatchPlan f = sdr::plan_batch(sw, sdr::BatchGeometry{bands, 16384, max_frames, max_frames / C + 2, false}, frames, 0, false, 256);
            CHECK(f.fft.reserve_cus == 48 && f.fft.reserve_forced);
        }
    // the launcher caps the rule's value at a share of the device and takes a forced one as it is: the plan says which it is
    static_assert(sdr::kReserveDeviceShare == 4 && sdr::kReserveMax * sdr::kReserveDeviceShare == 256, "64 CUs are a quarter of the device the rule was measured on");
    CHECK(!plan(def, 1, 16384, 8192).fft.reserve_forced && !plan(def, 1, 4096, 8192).fft.reserve_forced);

    // the forced switch: every k_fft_r32 launch takes it as it is - below the rule's smallest batch, with the chains, beyond
    // any device's CU count (the launcher keeps one workgroup)
    for (int forced : {0, 1, 48, 255, 300}) {
        sdr::Switches sw;
        sw.fft_reserve = forced;
        for (int frames : {1024, 1031, 2048, 8192})
            for (int bands : {1, 3})
                CHECK(plan(sw, bands, 16384, frames).fft.r32 && plan(sw, bands, 16384, frames).fft.reserve_cus == forced && plan(sw, bands, 16384, frames).fft.reserve_forced);
        sw.noise_scan = false;
        CHECK(plan(sw, 1, 16384, 8192).fft.reserve_cus == forced);
        sw.fft_r32 = 1;
        CHECK(plan(sw, 1, 16384, 1).fft.r32 && plan(sw, 1, 16384, 1).fft.reserve_cus == forced);
    }
    // ... read from the environment in read_switches, -1 (the rule) when unset or negative
    {
        unsetenv("SDR_FFT_RESERVE");
        CHECK(sdr::read_switches().fft_reserve == -1);
        setenv("SDR_FFT_RESERVE", "48", 1);
        CHECK(sdr::read_switches().fft_reserve == 48);
        setenv("SDR_FFT_RESERVE", "0", 1);
        CHECK(sdr::read_switches().fft_reserve == 0);
        setenv("SDR_FFT_RESERVE", "-1", 1);
        CHECK(sdr::read_switches().fft_reserve == -1);
        unsetenv("SDR_FFT_RESERVE");
    }

    // capture equals eager for the same geometry: a captured batch plans the slots an eager batch of that length touches at
    // most (n_chunks + 1), and the reserve follows from them by the same rule
    for (int bands : {1, 3, 24})
        for (int frames : {1024, 2048, 4096, 8192}) {
            const sdr::BatchPlan cap = plan(def, bands, 16384, frames, 0, true);
            CHECK(cap.fft.r32 == plan(def, bands, 16384, frames).fft.r32);
            if ((long)frames * bands < sdr::kReserveMinFrames) {
                CHECK(cap.fft.reserve_cus == 0);
                continue;
            }
            CHECK(cap.fft.reserve_cus == want(cap, bands));
            bool met = false;  // some eager cumulationCount touches as many slots: there the two plans agree in full
            for (int count0 = 0; count0 < C; count0++) {
                const sdr::BatchPlan e = plan(def, bands, 16384, frames, count0);
                if (e.n_slots == cap.n_slots) {
                    met = true;
                    CHECK(e.scan_parts == cap.scan_parts && e.fft.reserve_cus == cap.fft.reserve_cus);
                }
            }
            CHECK(met);
        }
    {
        sdr::Switches sw;
        sw.fft_reserve = 48;
        CHECK(plan(sw, 1, 16384, 1024, 0, true).fft.reserve_cus == 48);
    }

    std::printf(g_failures ? "FAILED %d\n" : "plan ok\n", g_failures);
    return g_failures ? 1 : 0;
}
