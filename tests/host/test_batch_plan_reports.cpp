// The batch plan with listener reports (sdrainer_amd/csrc/host/batch_plan.h, sdr_enable_reports): reports off is the plan of
// a bank that never heard of reports, field by field over the sweep tests/host/test_batch_plan_rows.cpp uses; reports on
// changes nothing of it and adds exactly the report launches - on the decode stage's stream, whatever stream the gather
// took - and only for a batch that has listener slots.  Built by tests/test_batch_plan_reports.py.  No GPU, no HIP.
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

// every field the plan had before reports
bool same_stages(const sdr::BatchPlan &a, const sdr::BatchPlan &b)
{
    for (int k = 0; k < sdr::K_COUNT; k++)
        if (a.stream[k] != b.stream[k])
            return false;
    return a.fft.r32 == b.fft.r32 && a.fft.fpw == b.fft.fpw && a.fft.wide_tap == b.fft.wide_tap && a.fft.two_phase == b.fft.two_phase &&
           a.fft.group_frames == b.fft.group_frames && a.fft.reserve_cus == b.fft.reserve_cus && a.fft.reserve_forced == b.fft.reserve_forced &&
           a.noise_scan == b.noise_scan && a.force_exact == b.force_exact && a.var_mfma == b.var_mfma && a.wm_wpb == b.wm_wpb &&
           a.bound == b.bound && a.bound_done == b.bound_done && a.scan_parts == b.scan_parts && a.n_slots == b.n_slots &&
           a.n_chunks == b.n_chunks && a.new_count == b.new_count && a.refine == b.refine && a.rows == b.rows && a.rows_stream == b.rows_stream;
}

void slots()
{
    // the two profile slots sit behind the rows kernel's; the stages and the rows kernel keep their numbers
    static_assert(sdr::K_COUNT == 8 && sdr::K_CUM_ROWS == 8 && sdr::K_PROFILE_COUNT == 9, "the slots of before");
    static_assert(sdr::K_LISTEN_REPORT == 9 && sdr::K_REPORT_MARKS == 10 && sdr::K_PROFILE_SLOTS == 11, "report slots");
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
                        for (int windowed = 0; windowed < 2; windowed++)
                            for (int columns : {0, 64})
                                for (int max_slots : {0, 16, 256}) {
                                    const sdr::BatchGeometry g{bands, n, 8192, 8192 / SDR_CUMULATION_SIZE + 2, true};
                                    const sdr::BatchPlan today = sdr::plan_batch(sw, g, frames, count0, capturing != 0, max_slots, windowed != 0, columns);
                                    const sdr::BatchPlan no = sdr::plan_batch(sw, g, frames, count0, capturing != 0, max_slots, windowed != 0, columns, false);
                                    CHECK(same_stages(today, no) && !today.reports && !no.reports);
                                    const sdr::BatchPlan yes = sdr::plan_batch(sw, g, frames, count0, capturing != 0, max_slots, windowed != 0, columns, true);
                                    CHECK(same_stages(today, yes));
                                    CHECK(yes.reports == (max_slots > 0));
                                    CHECK(yes.reports_stream == sdr::S_LISTEN && yes.reports_stream == yes.stream[sdr::K_LISTEN_DECODE]);
                                    (yes.reports ? on : off)++;
                                }
    CHECK(on > 0 && off > 0);
    // the small plan moves the gather to the peaks stream: the reports stay with the decoder
    const sdr::BatchPlan small = sdr::plan_batch(sw, sdr::BatchGeometry{1, 512, 256, 4, true}, 130, 0, false, 70, false, 0, true);
    CHECK(small.stream[sdr::K_LISTEN_GATHER] == sdr::S_PEAKS && small.reports && small.reports_stream == sdr::S_LISTEN);
    // both report kernels are part of the listen graph of a capture, and of no other
    const sdr::BatchPlan cap = sdr::plan_batch(sw, sdr::BatchGeometry{1, 4096, 256, 4, true}, 130, 0, true, 8, false, 0, true);
    for (int graph = 0; graph < sdr::N_GRAPHS; graph++)
        CHECK(sdr::in_graph(cap, sdr::K_LISTEN_DECODE, graph) == (graph == cap.reports_stream));
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
