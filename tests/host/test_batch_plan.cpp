// Host-only test of the batch plan (sdrainer_amd/csrc/host/batch_plan.h - the code the library runs, not a copy): every
// rule the scheduler applies to a batch, pinned at the boundaries where it switches, each switch forced both ways, and
// invariants over a sweep of geometries.  The `legacy_*` functions are the rules as the launchers and the scheduler
// applied them before the plan existed (k_fft_psd.hip use_r32, k_peaks.hip cum_bound_pays and the refinement's shape,
// k_noise_scan.hip scan_parts, the two slot counts of process_device_body): the plan must agree with them everywhere.
// Built by tests/test_batch_plan.py.  No GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

using sdr::BatchGeometry;
using sdr::BatchPlan;
using sdr::Refine;
using sdr::Switches;

constexpr int C = SDR_CUMULATION_SIZE;

BatchGeometry geom(int bands, int n, int max_batch_frames = 16384)
{
    return BatchGeometry{bands, n, max_batch_frames, max_batch_frames / C + 2};
}

BatchPlan plan(int bands, int n, int n_frames, int count0 = 0, bool cap = false, int max_slots = 16, const Switches &sw = Switches())
{
    return sdr::plan_batch(sw, geom(bands, n), n_frames, count0, cap, max_slots);
}

// ---- the rules as they were written before the plan (sdr_device.h chunks_completed is unchanged)
int chunks_completed(int count0, int n_frames)
{
    const int first_len = C - count0;
    return n_frames >= first_len ? 1 + (n_frames - first_len) / C : 0;
}
bool legacy_use_r32(int mode, int logn, int n_frames, int n_bands, int tap_n)
{
    return logn == 14 && tap_n <= 512 && (mode == 1 || (mode < 0 && (long)n_frames * n_bands >= 1024));
}
bool legacy_cum_bound_pays(int force, int n_frames, int n_bands, int n)
{
    if (force >= 0)
        return force != 0;
    return (double)n_frames * (double)n_bands * (double)n >= 64.0 * 1024.0 * 1024.0;
}
int legacy_scan_parts(int n_slots, int n_bands) { return (long)n_slots * n_bands < 64 ? 2 : 1; }
bool legacy_wide(int wide_env, int n, int n_chunks, int n_bands) { return wide_env >= 0 ? wide_env != 0 : (n >= 4096 && (long)n_chunks * n_bands >= 64); }
int legacy_scan_slots(int count0, int n_frames, bool cap)
{
    int scan_slots = 1;
    if (n_frames >= C - count0)
        scan_slots = 1 + (n_frames - (C - count0) + C - 1) / C;
    if (cap)
        scan_slots = chunks_completed(C - 1, n_frames) + 1;
    return scan_slots;
}
void legacy_cum_counts(int count0, int n_frames, bool cap, int *n_slots_c, int *n_chunks)
{
    const int first_len = C - count0;
    *n_slots_c = 1;
    *n_chunks = 0;
    if (n_frames >= first_len) {
        *n_chunks = 1 + (n_frames - first_len) / C;
        const int rem = (n_frames - first_len) % C;
        *n_slots_c = *n_chunks + (rem > 0 ? 1 : 0);
    }
    if (cap) {
        *n_chunks = chunks_completed(C - 1, n_frames);
        *n_slots_c = *n_chunks + 1;
    }
}
int legacy_log2(int n)
{
    int s = 0;
    while ((1 << s) < n)
        s++;
    return s;
}

void test_switches()
{
    const char *names[] = {"SDR_NOISE_PATH", "SDR_NOISE_FORCE_EXACT", "SDR_FFT_R32",   "SDR_FFT_FPW",     "SDR_CUM_BOUND", "SDR_REFINE_WIDE",
                           "SDR_VAR_MFMA",   "SDR_WM_WPB",            "SDR_NO_OVERLAP", "SDR_GRAPH_DEBUG", "SDR_DIAG_SKIP", "SDR_DIAG_PLAN"};
    for (const char *n : names)
        unsetenv(n);
    Switches d = sdr::read_switches();
    CHECK(d.noise_scan && d.force_exact == 0 && d.fft_r32 == -1 && d.fft_fpw == 0 && d.cum_bound == -1 && d.refine_wide == -1 &&
          d.var_mfma == -1 && d.wm_wpb == 0 && !d.no_overlap && !d.graph_debug && d.diag_skip == 0);
    for (int k = 0; k < sdr::K_COUNT; k++)
        CHECK(d.diag_plan[k] == -1);

    setenv("SDR_NOISE_PATH", "chains", 1);
    CHECK(!sdr::read_switches().noise_scan);
    setenv("SDR_NOISE_PATH", "scan", 1);
    CHECK(sdr::read_switches().noise_scan);
    setenv("SDR_NOISE_PATH", "chainsx", 1);
    CHECK(sdr::read_switches().noise_scan);
    unsetenv("SDR_NOISE_PATH");

    setenv("SDR_NOISE_FORCE_EXACT", "3", 1);
    CHECK(sdr::read_switches().force_exact == 3);
    unsetenv("SDR_NOISE_FORCE_EXACT");

    // SDR_FFT_R32: any non-zero number forces the 32-point kernel
    const struct { const char *v; int want; } r32[] = {{"0", 0}, {"1", 1}, {"2", 1}, {"-1", 1}, {"x", 0}};
    for (auto t : r32) {
        setenv("SDR_FFT_R32", t.v, 1);
        CHECK(sdr::read_switches().fft_r32 == t.want);
    }
    unsetenv("SDR_FFT_R32");

    // SDR_FFT_FPW: clamped to 1 - 64
    const struct { const char *v; int want; } fpw[] = {{"0", 1}, {"1", 1}, {"4", 4}, {"64", 64}, {"65", 64}, {"-3", 1}};
    for (auto t : fpw) {
        setenv("SDR_FFT_FPW", t.v, 1);
        CHECK(sdr::read_switches().fft_fpw == t.want);
    }
    unsetenv("SDR_FFT_FPW");

    // the three 0 / 1 switches: a negative value leaves the choice to the rule
    const char *tri[] = {"SDR_CUM_BOUND", "SDR_REFINE_WIDE", "SDR_VAR_MFMA"};
    const struct { const char *v; int want; } tv[] = {{"0", 0}, {"1", 1}, {"7", 1}, {"-1", -1}, {"x", 0}};
    for (const char *n : tri) {
        for (auto t : tv) {
            setenv(n, t.v, 1);
            const Switches s = sdr::read_switches();
            const int got = !strcmp(n, "SDR_CUM_BOUND") ? s.cum_bound : !strcmp(n, "SDR_REFINE_WIDE") ? s.refine_wide : s.var_mfma;
            CHECK(got == t.want);
        }
        unsetenv(n);
    }

    const struct { const char *v; int want; } wpb[] = {{"0", 0}, {"-2", 0}, {"3", 3}, {"12", 12}};
    for (auto t : wpb) {
        setenv("SDR_WM_WPB", t.v, 1);
        CHECK(sdr::read_switches().wm_wpb == t.want);
    }
    unsetenv("SDR_WM_WPB");

    setenv("SDR_NO_OVERLAP", "1", 1);
    CHECK(sdr::read_switches().no_overlap);
    setenv("SDR_NO_OVERLAP", "0", 1);
    CHECK(!sdr::read_switches().no_overlap);
    setenv("SDR_NO_OVERLAP", "10", 1);
    CHECK(sdr::read_switches().no_overlap);
    unsetenv("SDR_NO_OVERLAP");

    setenv("SDR_GRAPH_DEBUG", "", 1);
    CHECK(sdr::read_switches().graph_debug);
    unsetenv("SDR_GRAPH_DEBUG");

    setenv("SDR_DIAG_SKIP", "5", 1);
    setenv("SDR_DIAG_PLAN", "0123x", 1);
    const Switches g = sdr::read_switches();
#if defined(SDR_DIAG)
    CHECK(g.diag_skip == 5);
    CHECK(g.diag_plan[0] == 0 && g.diag_plan[1] == 1 && g.diag_plan[2] == 2 && g.diag_plan[3] == 3 && g.diag_plan[4] == -1);
    setenv("SDR_DIAG_PLAN", "00000004", 1);  // (4 is no stream: the override stops there)
    const Switches g2 = sdr::read_switches();
    for (int k = 0; k < sdr::K_COUNT; k++)
        CHECK(g2.diag_plan[k] == (k < 7 ? 0 : -1));
#else
    CHECK(g.diag_skip == 0 && g.diag_plan[0] == -1);  // (read by -DSDR_DIAG builds only)
#endif
    unsetenv("SDR_DIAG_SKIP");
    unsetenv("SDR_DIAG_PLAN");
    std::printf("switches ok\n");
}

void test_fft()
{
    // by frames per launch: 1024 on (frames x bands)
    CHECK(!plan(1, 16384, 1023).fft.r32);
    CHECK(plan(1, 16384, 1024).fft.r32);
    CHECK(!plan(4, 16384, 255).fft.r32);
    CHECK(plan(4, 16384, 256).fft.r32);
    CHECK(plan(24, 16384, 64).fft.r32);
    // while the listener slots fit its tap: 512
    CHECK(plan(1, 16384, 2048, 0, false, 512).fft.r32);
    CHECK(!plan(1, 16384, 2048, 0, false, 513).fft.r32);
    // N = 16384 only
    for (int n = 512; n <= 8192; n *= 2)
        CHECK(!plan(1, n, 8192).fft.r32);
    // the wide tap: k_fft_r32 with listeners
    CHECK(plan(1, 16384, 2048, 0, false, 1).fft.wide_tap);
    CHECK(!plan(1, 16384, 2048, 0, false, 0).fft.wide_tap);
    CHECK(plan(1, 16384, 2048, 0, false, 0).fft.r32);
    CHECK(!plan(1, 16384, 1023, 0, false, 16).fft.wide_tap);
    CHECK(!plan(1, 16384, 2048, 0, false, 513).fft.wide_tap);
    // forced: SDR_FFT_R32 = 0 / 1 (never beyond the slots it serves, never at another N)
    Switches on, off;
    on.fft_r32 = 1;
    off.fft_r32 = 0;
    CHECK(plan(1, 16384, 1, 0, false, 16, on).fft.r32);
    CHECK(plan(1, 16384, 1, 0, false, 16, on).fft.wide_tap);
    CHECK(!plan(1, 16384, 1, 0, false, 513, on).fft.r32);
    CHECK(!plan(1, 8192, 8192, 0, false, 16, on).fft.r32);
    CHECK(!plan(1, 16384, 8192, 0, false, 16, off).fft.r32);
    CHECK(!plan(1, 16384, 8192, 0, false, 16, off).fft.wide_tap);
    // frames per workgroup: passed through (0 = the kernel's default)
    CHECK(plan(1, 4096, 2048).fft.fpw == 0);
    Switches fpw;
    fpw.fft_fpw = 4;
    CHECK(plan(1, 4096, 2048, 0, false, 16, fpw).fft.fpw == 4);
    CHECK(sdr::fft_choice(fpw, 16384, 2048, 1, 16).r32 && sdr::fft_choice(fpw, 16384, 2048, 1, 16).fpw == 4);
    std::printf("fft ok\n");
}

void test_bound()
{
    // 64 M samples per batch (frames x bands x N)
    CHECK(!plan(1, 16384, 4095).bound);
    CHECK(plan(1, 16384, 4096).bound);
    CHECK(!plan(8, 8192, 1023).bound);
    CHECK(plan(8, 8192, 1024).bound);
    CHECK(!plan(1, 4096, 16383).bound);
    CHECK(plan(1, 4096, 16384).bound);
    // the scan forms the unit counts on the scan path only
    CHECK(plan(1, 16384, 4096).bound_done);
    CHECK(!plan(1, 16384, 4095).bound_done);
    Switches chains;
    chains.noise_scan = false;
    CHECK(plan(1, 16384, 4096, 0, false, 16, chains).bound);
    CHECK(!plan(1, 16384, 4096, 0, false, 16, chains).bound_done);
    CHECK(!plan(1, 16384, 4096, 0, false, 16, chains).noise_scan);
    // forced
    Switches on, off;
    on.cum_bound = 1;
    off.cum_bound = 0;
    CHECK(plan(1, 512, 1, 0, false, 16, on).bound && plan(1, 512, 1, 0, false, 16, on).bound_done);
    CHECK(!plan(1, 16384, 8192, 0, false, 16, off).bound && !plan(1, 16384, 8192, 0, false, 16, off).bound_done);
    CHECK(plan(1, 16384, 8192, 0, false, 16, off).refine == Refine::NONE);
    std::printf("bound ok\n");
}

void test_parts()
{
    // n_slots x bands: 63 -> 2, 64 -> 1
    const BatchPlan a = plan(1, 16384, 63 * C), b = plan(1, 16384, 63 * C + 1);
    CHECK(a.n_slots == 63 && a.scan_parts == 2);
    CHECK(b.n_slots == 64 && b.scan_parts == 1);
    const BatchPlan c = plan(8, 16384, 7 * C), d = plan(8, 16384, 7 * C + 1);
    CHECK(c.n_slots == 7 && c.scan_parts == 2);
    CHECK(d.n_slots == 8 && d.scan_parts == 1);
    CHECK(plan(1, 16384, 2048).scan_parts == 2);  // (config 3 at 2048 frames: 21 slots)
    CHECK(plan(1, 16384, 8192).scan_parts == 1);  // (83 slots)
    std::printf("parts ok\n");
}

void test_gather()
{
    // B x N <= 8192: the gather moves to the peaks stream, outside a capture
    CHECK(plan(1, 8192, 64).stream[sdr::K_LISTEN_GATHER] == sdr::S_PEAKS);
    CHECK(plan(2, 4096, 64).stream[sdr::K_LISTEN_GATHER] == sdr::S_PEAKS);
    CHECK(plan(1, 16384, 64).stream[sdr::K_LISTEN_GATHER] == sdr::S_LISTEN);
    CHECK(plan(3, 4096, 64).stream[sdr::K_LISTEN_GATHER] == sdr::S_LISTEN);
    CHECK(sdr::plan_batch(Switches(), geom(1, 8193), 64, 0, false, 16).stream[sdr::K_LISTEN_GATHER] == sdr::S_LISTEN);
    CHECK(sdr::plan_batch(Switches(), geom(3, 2731), 64, 0, false, 16).stream[sdr::K_LISTEN_GATHER] == sdr::S_LISTEN);  // (8193)
    CHECK(plan(1, 8192, 64, 0, true).stream[sdr::K_LISTEN_GATHER] == sdr::S_LISTEN);
    CHECK(plan(1, 512, 64, 0, true).stream[sdr::K_LISTEN_GATHER] == sdr::S_LISTEN);
    // everything else, always
    const int rest[sdr::K_COUNT] = {sdr::S_FFT, sdr::S_NOISE, sdr::S_NOISE, sdr::S_PEAKS, -1, sdr::S_PEAKS, sdr::S_PEAKS, sdr::S_LISTEN};
    for (bool cap : {false, true})
        for (int n : {512, 8192, 16384})
            for (int k = 0; k < sdr::K_COUNT; k++)
                if (k != sdr::K_LISTEN_GATHER)
                    CHECK(plan(1, n, 100, 0, cap).stream[k] == rest[k]);
    // SDR_DIAG_PLAN: over the plan's table, the gather move included
    Switches diag;
    diag.diag_plan[sdr::K_FFT] = sdr::S_NOISE;
    diag.diag_plan[sdr::K_LISTEN_GATHER] = sdr::S_LISTEN;
    const BatchPlan p = plan(1, 4096, 64, 0, false, 16, diag);
    CHECK(p.stream[sdr::K_FFT] == sdr::S_NOISE && p.stream[sdr::K_LISTEN_GATHER] == sdr::S_LISTEN && p.stream[sdr::K_CUMULATE] == sdr::S_PEAKS);
    std::printf("gather ok\n");
}

void test_refine()
{
    // N = 2048 / 4096 (bound by size, many cumulations)
    CHECK(plan(1, 2048, 32768).bound && plan(1, 2048, 32768).refine == Refine::NARROW);
    CHECK(plan(1, 4096, 16384).bound && plan(1, 4096, 16384).refine == Refine::WIDE);
    // n_chunks x bands: 63 / 64
    CHECK(plan(1, 16384, 63 * C).n_chunks == 63 && plan(1, 16384, 63 * C).refine == Refine::NARROW);
    CHECK(plan(1, 16384, 64 * C).n_chunks == 64 && plan(1, 16384, 64 * C).refine == Refine::WIDE);
    CHECK(plan(8, 16384, 7 * C + 99).n_chunks == 7 && plan(8, 16384, 7 * C + 99).refine == Refine::NARROW);
    CHECK(plan(8, 16384, 8 * C).refine == Refine::WIDE);
    CHECK(plan(1, 16384, 4096).refine == Refine::NARROW);  // (40 cumulations)
    CHECK(plan(1, 16384, 4095).refine == Refine::NONE);
    // under capture the grid's chunk count decides
    CHECK(plan(1, 16384, 63 * C + 1, 0, true).n_chunks == 64 && plan(1, 16384, 63 * C + 1, 0, true).refine == Refine::WIDE);
    // forced (with the bound forced on too, on a batch far too short for either)
    Switches w, nw;
    w.cum_bound = nw.cum_bound = 1;
    w.refine_wide = 1;
    nw.refine_wide = 0;
    CHECK(plan(1, 512, 100, 0, false, 16, w).refine == Refine::WIDE);
    CHECK(plan(1, 16384, 64 * C, 0, false, 16, nw).refine == Refine::NARROW);
    Switches w_only;
    w_only.refine_wide = 1;
    CHECK(plan(1, 512, 100, 0, false, 16, w_only).refine == Refine::NONE);  // (no bound: nothing to refine)
    std::printf("refine ok\n");
}

void test_counts()
{
    // literal values at the chunk ends
    struct Case { int count0, n, chunks, slots, new_count; };
    const Case cases[] = {{0, 1, 0, 1, 1},    {0, 99, 0, 1, 99},   {0, 100, 1, 1, 0},   {0, 101, 1, 2, 1},   {0, 199, 1, 2, 99},
                          {0, 200, 2, 2, 0},  {0, 201, 2, 3, 1},   {1, 1, 0, 1, 2},     {1, 98, 0, 1, 99},   {1, 99, 1, 1, 0},
                          {1, 100, 1, 2, 1},  {1, 199, 2, 2, 0},   {1, 200, 2, 3, 1},   {99, 1, 1, 1, 0},    {99, 2, 1, 2, 1},
                          {99, 100, 1, 2, 99}, {99, 101, 2, 2, 0}, {99, 102, 2, 3, 1},  {0, 8192, 81, 82, 92}, {99, 8192, 82, 83, 91}};
    for (const Case &t : cases) {
        const BatchPlan p = plan(1, 16384, t.n, t.count0);
        CHECK(p.n_chunks == t.chunks && p.n_slots == t.slots && p.new_count == t.new_count);
        if (!(p.n_chunks == t.chunks && p.n_slots == t.slots && p.new_count == t.new_count))
            std::printf("  count0 %d n %d: chunks %d slots %d new %d\n", t.count0, t.n, p.n_chunks, p.n_slots, p.new_count);
    }
    // under capture: the most chunks a batch of this length completes (from count0 = 99), plus the open slot, whatever count0
    struct Cap { int n, chunks, slots; };
    const Cap caps[] = {{1, 1, 2}, {99, 1, 2}, {100, 1, 2}, {101, 2, 3}, {200, 2, 3}, {201, 3, 4}, {2048, 21, 22}, {8192, 82, 83}};
    for (const Cap &t : caps)
        for (int count0 : {0, 1, 99}) {
            const BatchPlan p = plan(1, 16384, t.n, count0, true);
            CHECK(p.n_chunks == t.chunks && p.n_slots == t.slots);
            CHECK(p.new_count == (count0 + t.n) % C);
        }
    // every count0 and batch length around the chunk ends against the code the plan replaced
    for (int count0 = 0; count0 < C; count0++)
        for (int n = 1; n <= 4 * C + 3; n++)
            for (bool cap : {false, true}) {
                const BatchPlan p = plan(1, 16384, n, count0, cap);
                int slots_c, chunks;
                legacy_cum_counts(count0, n, cap, &slots_c, &chunks);
                CHECK(p.n_chunks == chunks && p.n_slots == slots_c && p.n_slots == legacy_scan_slots(count0, n, cap));
                if (!cap)
                    CHECK(p.n_chunks == chunks_completed(count0, n));
                CHECK(p.new_count == (count0 + n) % C);
            }
    std::printf("counts ok\n");
}

void test_forced_rest()
{
    // the chains' two choices
    CHECK(plan(1, 16384, 4095).var_mfma);
    CHECK(!plan(1, 16384, 4096).var_mfma);
    Switches m1, m0;
    m1.var_mfma = 1;
    m0.var_mfma = 0;
    CHECK(plan(1, 16384, 8192, 0, false, 16, m1).var_mfma);
    CHECK(!plan(1, 16384, 64, 0, false, 16, m0).var_mfma);
    Switches wpb;
    wpb.wm_wpb = 5;
    CHECK(plan(1, 16384, 64).wm_wpb == 0 && plan(1, 16384, 64, 0, false, 16, wpb).wm_wpb == 5);
    // the scan's literal fallback
    Switches fe;
    fe.force_exact = 3;
    CHECK(plan(1, 16384, 64).force_exact == 0 && plan(1, 16384, 64, 0, false, 16, fe).force_exact == 3);
    CHECK(plan(1, 16384, 64).noise_scan);
    std::printf("forced ok\n");
}

// The order of a batch's stages: who waits for whom, which stage stands for its stream when a set is reused, which graph
// a kernel belongs to - literal tables at the plans that differ.
void test_order()
{
    using namespace sdr;
    struct Dep { int k, dep; };
    auto deps_are = [](const sdr::StageDeps &s, std::initializer_list<Dep> want) {
        bool same = s.n == (int)want.size() && s.n <= sdr::StageDeps::kMax;
        int i = 0;
        for (const Dep &w : want) {
            same = same && i < s.n && s.d[i].k == w.k && s.d[i].dep == w.dep;
            i++;
        }
        return same;
    };
    // the dependency list in issue order: the default plan (no bound at this length), with and without the peak scan
    const BatchPlan def = plan(1, 16384, 2048);
    CHECK(!def.bound_done);
    CHECK(deps_are(stage_deps(def, true), {{K_WINDOW_MEANS, K_FFT},
                                           {K_NOISE_STATS, K_WINDOW_MEANS},
                                           {K_THRESHOLDS, K_NOISE_STATS},
                                           {K_LISTEN_GATHER, K_THRESHOLDS},
                                           {K_LISTEN_GATHER, K_FFT},
                                           {K_LISTEN_DECODE, K_LISTEN_GATHER},
                                           {K_CUMULATE, K_FFT},
                                           {K_FIND_PEAKS, K_CUMULATE},
                                           {K_FIND_PEAKS, K_THRESHOLDS}}));
    CHECK(deps_are(stage_deps(def, false), {{K_WINDOW_MEANS, K_FFT},
                                            {K_NOISE_STATS, K_WINDOW_MEANS},
                                            {K_THRESHOLDS, K_NOISE_STATS},
                                            {K_LISTEN_GATHER, K_THRESHOLDS},
                                            {K_LISTEN_GATHER, K_FFT},
                                            {K_LISTEN_DECODE, K_LISTEN_GATHER},
                                            {K_CUMULATE, K_FFT},
                                            {K_FIND_PEAKS, K_CUMULATE}}));
    // bound_done: the cumulation also waits for the scan (the window-means stage), behind its wait for the FFT
    const BatchPlan bd = plan(1, 16384, 8192);
    CHECK(bd.bound_done);
    CHECK(deps_are(stage_deps(bd, true), {{K_WINDOW_MEANS, K_FFT},
                                          {K_NOISE_STATS, K_WINDOW_MEANS},
                                          {K_THRESHOLDS, K_NOISE_STATS},
                                          {K_LISTEN_GATHER, K_THRESHOLDS},
                                          {K_LISTEN_GATHER, K_FFT},
                                          {K_LISTEN_DECODE, K_LISTEN_GATHER},
                                          {K_CUMULATE, K_FFT},
                                          {K_CUMULATE, K_WINDOW_MEANS},
                                          {K_FIND_PEAKS, K_CUMULATE},
                                          {K_FIND_PEAKS, K_THRESHOLDS}}));
    Switches chains;
    chains.noise_scan = false;
    const BatchPlan ch = plan(1, 16384, 8192, 0, false, 16, chains);  // (bounded, but k_cum_bound forms the counts on the peaks stream)
    CHECK(ch.bound && !ch.bound_done && stage_deps(ch, true).n == 9 && stage_deps(ch, false).n == 8);
    // the list does not depend on the streams: the small-geometry plan has the default one
    CHECK(stage_deps(plan(1, 512, 2048), true).n == 9 && stage_deps(plan(1, 512, 2048), true).d[3].k == K_LISTEN_GATHER);

    // set reuse: the last stage issued on each stream stands for it; the FFT's stream is left out
    int s[N_STAGES];
    set_reuse_stages(def, s);
    CHECK(s[S_FFT] == -1 && s[S_NOISE] == K_NOISE_STATS && s[S_LISTEN] == K_LISTEN_DECODE && s[S_PEAKS] == K_FIND_PEAKS);
    set_reuse_stages(bd, s);
    CHECK(s[S_FFT] == -1 && s[S_NOISE] == K_NOISE_STATS && s[S_LISTEN] == K_LISTEN_DECODE && s[S_PEAKS] == K_FIND_PEAKS);
    // small geometry: the gather runs on S_PEAKS, decode alone stands for S_LISTEN
    const BatchPlan small = plan(1, 4096, 2048);
    CHECK(small.stream[K_LISTEN_GATHER] == S_PEAKS);
    set_reuse_stages(small, s);
    CHECK(s[S_FFT] == -1 && s[S_NOISE] == K_NOISE_STATS && s[S_LISTEN] == K_LISTEN_DECODE && s[S_PEAKS] == K_FIND_PEAKS);
    // a plan that moves stages (SDR_DIAG_PLAN): a stream without a stage has none, a stage beside the FFT is left out
    Switches moved;
    moved.diag_plan[K_LISTEN_DECODE] = S_PEAKS;  // (the gather is on S_PEAKS at this geometry: nothing is left on S_LISTEN)
    moved.diag_plan[K_NOISE_STATS] = S_FFT;
    set_reuse_stages(plan(1, 4096, 2048, 0, false, 16, moved), s);
    CHECK(s[S_FFT] == -1 && s[S_NOISE] == K_WINDOW_MEANS && s[S_LISTEN] == -1 && s[S_PEAKS] == K_FIND_PEAKS);
    Switches one;  // SDR_NO_OVERLAP is not a plan matter (every stream IS the caller's), but a plan on one stream waits for nothing
    for (int k = 0; k < K_COUNT; k++)
        one.diag_plan[k] = S_FFT;
    set_reuse_stages(plan(1, 4096, 2048, 0, false, 16, one), s);
    CHECK(s[S_FFT] == -1 && s[S_NOISE] == -1 && s[S_LISTEN] == -1 && s[S_PEAKS] == -1);

    // graph membership: every kernel against every graph, under capture (the gather stays on S_LISTEN there)
    CHECK(G_THRESHOLDS == 4 && N_GRAPHS == 5);
    const int graph_of[K_COUNT] = {/* fft */ S_FFT,       /* window means */ S_NOISE, /* noise stats */ S_NOISE, /* thresholds */ G_THRESHOLDS,
                                   /* gather */ S_LISTEN, /* cumulate */ S_PEAKS,     /* find peaks */ S_PEAKS,  /* decode */ S_LISTEN};
    for (int n : {512, 16384}) {
        const BatchPlan cap = plan(1, n, 2048, 0, true);
        for (int k = 0; k < K_COUNT; k++)
            for (int g = 0; g < N_GRAPHS; g++)
                CHECK(in_graph(cap, k, g) == (g == graph_of[k]));
    }
    // ... and by stream, not by a table: a moved stage follows its stream, the thresholds stay in their own graph
    Switches mv;
    mv.diag_plan[K_LISTEN_GATHER] = S_PEAKS;
    mv.diag_plan[K_THRESHOLDS] = S_NOISE;
    const BatchPlan mvp = plan(1, 16384, 2048, 0, true, 16, mv);
    for (int g = 0; g < N_GRAPHS; g++) {
        CHECK(in_graph(mvp, K_LISTEN_GATHER, g) == (g == S_PEAKS));
        CHECK(in_graph(mvp, K_THRESHOLDS, g) == (g == G_THRESHOLDS));
    }
    std::printf("order ok\n");
}

// Invariants and the rules before the plan, over geometries, lengths, phases, listener counts and switch settings.
void test_sweep()
{
    Switches sws[8];
    sws[1].noise_scan = false;
    sws[2].cum_bound = 1;
    sws[2].refine_wide = 0;
    sws[3].cum_bound = 0;
    sws[4].fft_r32 = 1;
    sws[4].cum_bound = 1;
    sws[4].refine_wide = 1;
    sws[5].fft_r32 = 0;
    sws[6].noise_scan = false;
    sws[6].cum_bound = 1;
    sws[6].var_mfma = 0;
    sws[7].fft_fpw = 2;
    long plans = 0;
    for (const Switches &sw : sws)
        for (int bands : {1, 2, 3, 8, 24})
            for (int n = 512; n <= 16384; n *= 2)
                for (int frames : {1, 63, 64, 99, 100, 101, 255, 256, 1023, 1024, 2048, 4095, 4096, 6300, 6400, 8192, 16384})
                    for (int count0 : {0, 1, 50, 99})
                        for (bool cap : {false, true})
                            for (int slots : {0, 1, 256, 512, 513}) {
                                const BatchGeometry g = geom(bands, n, 16384);
                                const BatchPlan p = sdr::plan_batch(sw, g, frames, count0, cap, slots);
                                plans++;
                                // the scan and the cumulation see one slot count and one parts value, within the buffers
                                int slots_c, chunks;
                                legacy_cum_counts(count0, frames, cap, &slots_c, &chunks);
                                CHECK(p.n_slots == slots_c && p.n_slots == legacy_scan_slots(count0, frames, cap) && p.n_chunks == chunks);
                                CHECK(p.scan_parts == legacy_scan_parts(p.n_slots, bands));
                                CHECK(p.n_chunks <= p.n_slots && p.n_slots <= g.max_chunks);
                                // the bound and its refinement
                                const bool bound = legacy_cum_bound_pays(sw.cum_bound, frames, bands, n);
                                CHECK(p.bound == bound && p.bound_done == (sw.noise_scan && bound));
                                CHECK(p.refine == (!bound ? Refine::NONE : legacy_wide(sw.refine_wide, n, p.n_chunks, bands) ? Refine::WIDE : Refine::NARROW));
                                // the FFT: a wide tap implies k_fft_r32 and listeners
                                CHECK(p.fft.r32 == legacy_use_r32(sw.fft_r32, legacy_log2(n), frames, bands, slots));
                                CHECK(p.fft.wide_tap == (slots > 0 && p.fft.r32));
                                CHECK(!p.fft.wide_tap || (p.fft.r32 && slots > 0 && slots <= sdr::kR32MaxTap));
                                CHECK(p.fft.fpw == sw.fft_fpw);
                                // a plan made while capturing never moves the gather
                                if (cap)
                                    CHECK(p.stream[sdr::K_LISTEN_GATHER] == sdr::S_LISTEN);
                                else
                                    CHECK(p.stream[sdr::K_LISTEN_GATHER] == ((long)bands * n <= 8192 ? sdr::S_PEAKS : sdr::S_LISTEN));
                                CHECK(p.var_mfma == (sw.var_mfma >= 0 ? sw.var_mfma != 0 : frames < 4096));
                                if (g_failures > 20)
                                    return;
                            }
    CHECK(plans > 100000);
    std::printf("sweep ok\n");
}

}  // namespace

int main()
{
    test_switches();
    test_fft();
    test_bound();
    test_parts();
    test_gather();
    test_refine();
    test_counts();
    test_forced_rest();
    test_order();
    test_sweep();
    return g_failures ? 1 : 0;
}
