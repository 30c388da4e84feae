// The batch plan with waterfall rows (sdrainer_amd/csrc/host/batch_plan.h, sdr_enable_rows): rows off is the plan of a bank
// that never heard of rows, field by field over a sweep of geometries, batch lengths and cumulation phases; rows on changes
// nothing of it and adds exactly one stage - on the peaks stream, the cumulate step's, in front of the find-peaks stage's
// event - and only for a batch that completes a cumulation (a captured batch may at any replay).  Built by
// tests/test_batch_plan_rows.py.  No GPU, no HIP.
#include <cstdio>
#include <initializer_list>

#include "../../sdrainer_amd/csrc/host/batch_plan.h"

namespace {
int g_failed = 0;
#define CHECK(c)                                                \
    do {                                                        \
        if (!(c)) {                                             \
            printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
            g_failed++;                                         \
        }                                                       \
    } while (0)

// every field of today's plan
bool same_stages(const sdr::BatchPlan &a, const sdr::BatchPlan &b)
{
    for (int k = 0; k < sdr::K_COUNT; k++)
        if (a.stream[k] != b.stream[k])
            return false;
    return a.fft.r32 == b.fft.r32 && a.fft.fpw == b.fft.fpw && a.fft.wide_tap == b.fft.wide_tap && a.fft.two_phase == b.fft.two_phase &&
           a.fft.group_frames == b.fft.group_frames && a.fft.reserve_cus == b.fft.reserve_cus && a.fft.reserve_forced == b.fft.reserve_forced &&
           a.noise_scan == b.noise_scan && a.force_exact == b.force_exact && a.var_mfma == b.var_mfma && a.wm_wpb == b.wm_wpb &&
           a.bound == b.bound && a.bound_done == b.bound_done && a.scan_parts == b.scan_parts && a.n_slots == b.n_slots &&
           a.n_chunks == b.n_chunks && a.new_count == b.new_count && a.refine == b.refine;
}

void slots()
{
    // the profile slot sits behind the eight stages, which keep their numbers
    static_assert(sdr::K_COUNT == 8 && sdr::K_CUM_ROWS == 8 && sdr::K_PROFILE_COUNT == 9, "profile slots");
    static_assert(sdr::K_FFT == 0 && sdr::K_CUMULATE == 5 && sdr::K_FIND_PEAKS == 6 && sdr::K_LISTEN_DECODE == 7, "stage numbers");
}

void sweep()
{
    const sdr::Switches sw;
    int on = 0, off = 0;
    for (int n : {512, 4096, 8192, 16384, 32768, 65536})
        for (int bands : {1, 2, 24})
            for (int frames : {1, 30, 99, 100, 130, 250, 1024, 2048, 8192})
                for (int count0 : {0, 1, 50, 70, 99})
                    for (int capturing = 0; capturing < 2; capturing++)
                        for (int windowed = 0; windowed < 2; windowed++) {
                            const sdr::BatchGeometry g{bands, n, 8192, 8192 / SDR_CUMULATION_SIZE + 2, true};
                            const sdr::BatchPlan today = sdr::plan_batch(sw, g, frames, count0, capturing != 0, 16, windowed != 0);
                            const sdr::BatchPlan zero = sdr::plan_batch(sw, g, frames, count0, capturing != 0, 16, windowed != 0, 0);
                            CHECK(same_stages(today, zero) && !today.rows && !zero.rows);
                            for (int columns : {64, 1024}) {
                                const sdr::BatchPlan rows = sdr::plan_batch(sw, g, frames, count0, capturing != 0, 16, windowed != 0, columns);
                                CHECK(same_stages(today, rows));
                                const bool completes = capturing || (count0 + frames) / SDR_CUMULATION_SIZE > 0;
                                CHECK(rows.rows == completes);
                                CHECK(rows.rows_stream == sdr::S_PEAKS && rows.rows_stream == rows.stream[sdr::K_CUMULATE] &&
                                      rows.rows_stream == rows.stream[sdr::K_FIND_PEAKS]);
                                (rows.rows ? on : off)++;
                            }
                        }
    CHECK(on > 0 && off > 0);
}
}  // namespace

int main()
{
    slots();
    printf("slots %s\n", g_failed ? "FAILED" : "ok");
    const int before = g_failed;
    sweep();
    printf("sweep %s\n", g_failed == before ? "ok" : "FAILED");
    return g_failed ? 1 : 0;
}
