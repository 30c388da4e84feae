// host/batch_plan.h — every choice the scheduler makes for one batch (process_device_body, capi_process.hip), made in one
// place: which stream each kernel runs on, which FFT kernel runs, which noise-floor path, whether the cumulations are
// bounded and refined, the slot and chunk counts; and the order of its stages (stage_deps, set_reuse_stages, in_graph: who
// waits for whom, which stage stands for its stream when a buffer set is reused, which graph a kernel belongs to under
// capture).  The launchers receive these decisions as arguments and decide nothing.
//
// The environment switches that steer the pipeline are read here too, by read_switches(), once per bank (sdr_create).
// They select a second implementation of a stage for the tests (tests/test_forced_paths.py) or are measurement knobs;
// with none of them set every choice follows the batch's geometry.  Two test hooks stay outside, read at each call
// because tests toggle them within one process: SDR_READ_CUM_RAW (sdr_read_cumulation) and SDR_SELF_CHECK_ORDER
// (sdr_self_check, which has no bank).
//
// Pure C++: tests/host/test_batch_plan.cpp pins every rule at the boundaries where it switches, without a GPU.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>

#include "../../../include/sdrainer_hip.h"

namespace sdr {

enum KernelId {
    K_FFT = 0, K_WINDOW_MEANS, K_NOISE_STATS, K_THRESHOLDS, K_LISTEN_GATHER, K_CUMULATE, K_FIND_PEAKS, K_LISTEN_DECODE,
    K_COUNT
};
// k_cum_rows (the waterfall rows of sdr_enable_rows) is no stage of the plan's table - it rides on the find-peaks stage's
// stream and events - but it has a profile slot, behind the eight stages' (sdr_profile_read / sdr_kernel_name)
constexpr int K_CUM_ROWS = K_COUNT, K_PROFILE_COUNT = K_COUNT + 1;
// ... and so have the two kernels of sdr_enable_reports, which ride on the decode stage's stream and events (k_report.hip):
// slots behind the rows kernel's.  K_PROFILE_SLOTS counts every profile slot.
constexpr int K_LISTEN_REPORT = K_PROFILE_COUNT, K_REPORT_MARKS = K_PROFILE_COUNT + 1, K_PROFILE_SLOTS = K_PROFILE_COUNT + 2;
// the bank's streams: four = the hardware queues HIP gives a process; with six streams created (two unused!) the step was
// 0.49 ms instead of 0.25, with GPU_MAX_HW_QUEUES=8 and five or six in use 0.29-0.60
enum Stage { S_FFT = 0, S_NOISE, S_LISTEN, S_PEAKS, N_STAGES };

// k_fft_r32 serves at most this many listener slots: one per thread (fft_r32.h fft32::T)
constexpr int kR32MaxTap = 512;

struct Switches {
    bool noise_scan = true;  // SDR_NOISE_PATH=chains: FindNoiseFloor by the ordered float64 chains of rounds 1-4 (k_noise.hip)
    int force_exact = 0;     // SDR_NOISE_FORCE_EXACT=k: the scan's literal fallback for every frame (1) or every k-th one (tests)
    int fft_r32 = -1;        // SDR_FFT_R32=0 / 1: N = 16384 never / always on k_fft_r32 (-1: by batch size)
    int fft_fpw = 0;         // SDR_FFT_FPW: frames per workgroup of the 16-point kernels, 1 - 64 (0: the kernel's default)
    int cum_bound = -1;      // SDR_CUM_BOUND=0 / 1: bound-and-refine never / always (-1: by batch size)
    int refine_wide = -1;    // SDR_REFINE_WIDE=0 / 1: the refinement's workgroup shape (-1: by cumulations per batch)
    int fft_reserve = -1;    // SDR_FFT_RESERVE=k: CUs k_fft_r32's grid leaves free (-1: fft_reserve_cus' rule; measurement and tests)
    int var_mfma = -1;       // SDR_VAR_MFMA=0 / 1: the chains' variance kernel (-1: by batch length)
    int wm_wpb = 0;          // SDR_WM_WPB: windows per workgroup of the chains' window sums (0: launch_window_means' rule)
    int fft2p_group_mb = -1;  // SDR_FFT2P_GROUP_MB: N > 16384, MiB of float64 intermediate per frame group (0: the whole batch; -1: kFft2pGroupMiB)
    bool no_overlap = false;   // SDR_NO_OVERLAP=1: every stage on the caller's stream (kernel-by-kernel profiling)
    bool graph_debug = false;  // SDR_GRAPH_DEBUG: host-side timings of every sdr_graph_launch on stderr
    bool queue_debug = false;  // SDR_QUEUE_DEBUG: what the bank's hardware queue probe found (sdr_create, sdr_set_stream) on stderr
    // -DSDR_DIAG builds only (tools/abl): SDR_DIAG_SKIP = bit mask of kernel ids not to launch, to see which stage holds the
    // pipelined step up (results are wrong by construction); SDR_DIAG_PLAN = the stream of each kernel, one digit each
    int diag_skip = 0;
    int diag_plan[K_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1};  // (-1: the plan's own)
};

// a forced 0 / 1 (any value >= 0: on unless 0), or -1 when unset or negative
inline int tri_state(const char *e)
{
    if (!e)
        return -1;
    const int v = atoi(e);
    return v >= 0 ? (v != 0 ? 1 : 0) : -1;
}

inline Switches read_switches()
{
    Switches s;
    const char *e;
    if ((e = getenv("SDR_NOISE_PATH")))
        s.noise_scan = strcmp(e, "chains") != 0;
    if ((e = getenv("SDR_NOISE_FORCE_EXACT")))
        s.force_exact = atoi(e);
    if ((e = getenv("SDR_FFT_R32")))
        s.fft_r32 = atoi(e) ? 1 : 0;
    if ((e = getenv("SDR_FFT_FPW"))) {
        const int v = atoi(e);
        s.fft_fpw = v < 1 ? 1 : (v > 64 ? 64 : v);
    }
    s.cum_bound = tri_state(getenv("SDR_CUM_BOUND"));
    s.refine_wide = tri_state(getenv("SDR_REFINE_WIDE"));
    s.var_mfma = tri_state(getenv("SDR_VAR_MFMA"));
    if ((e = getenv("SDR_FFT_RESERVE")))
        s.fft_reserve = atoi(e) >= 0 ? atoi(e) : -1;
    if ((e = getenv("SDR_FFT2P_GROUP_MB")))
        s.fft2p_group_mb = atoi(e) >= 0 ? atoi(e) : -1;  // (measurement: tools/fft2p_bench.py)
    if ((e = getenv("SDR_WM_WPB")))
        s.wm_wpb = atoi(e) > 0 ? atoi(e) : 0;  // (development)
    e = getenv("SDR_NO_OVERLAP");
    s.no_overlap = e && e[0] == '1';
    s.graph_debug = getenv("SDR_GRAPH_DEBUG") != nullptr;
    s.queue_debug = getenv("SDR_QUEUE_DEBUG") != nullptr;
#if defined(SDR_DIAG)
    if ((e = getenv("SDR_DIAG_SKIP")))
        s.diag_skip = atoi(e);
    if ((e = getenv("SDR_DIAG_PLAN")))
        for (int k = 0; k < K_COUNT && e[k] >= '0' && e[k] < '0' + N_STAGES; k++)
            s.diag_plan[k] = e[k] - '0';
#endif
    return s;
}

// The noise-floor path of a bank of block size n: the one-pass scan (k_noise_scan.hip) unless the chains are asked for.
// Above N = 16384 a window holds more than the 64 JMAX = 1664 values one scan wave owns: the chains (k_noise.hip), which
// take any window, compute the noise floor there.
inline bool noise_scan_at(const Switches &sw, int n) { return sw.noise_scan && n <= 16384; }
// The chains' variance on the matrix pipe relies on the order in which it accumulates (sdr_self_check probes it at
// sdr_create).  Only banks that ASKED for the chains (SDR_NOISE_PATH=chains, SDR_VAR_MFMA=1) may take it: at N > 16384,
// where the chains are the default noise path, the variance runs on the vector ALU unless SDR_VAR_MFMA=1.
inline bool var_mfma_at(const Switches &sw, int n, int n_frames)
{
    if (sw.var_mfma >= 0)
        return sw.var_mfma != 0;
    return n <= 16384 && n_frames < 4096;
}
// may a bank of block size n launch the matrix-pipe variance kernel (then sdr_create probes it)?
inline bool may_use_matrix_pipe(const Switches &sw, int n) { return !noise_scan_at(sw, n) && (sw.var_mfma == 1 || (sw.var_mfma < 0 && n <= 16384)); }

// What the FFT kernels read: interleaved float32 I,Q, complex int16 (sc16.h) or complex 8-bit, signed or unsigned (iq8.h)
enum class InFormat { F32 = 0, SC16 = 1, CS8 = 2, CU8 = 3 };
constexpr bool is_iq8(InFormat f) { return f == InFormat::CS8 || f == InFormat::CU8; }

// Which FFT kernel runs a batch, and how.
struct FftChoice {
    bool r32 = false;       // N = 16384 on k_fft_r32 instead of the 16-point k_fft_psd<14>
    int fpw = 0;            // the 16-point kernels: frames per workgroup asked for (0: kDefaultFpw; frames_per_wg is what runs)
    bool wide_tap = false;  // the kernel leaves the wide tap (psd at bin - 1, bin, bin + 1 of every listener: k_cum_refine reads it)
    bool two_phase = false;  // N = 32768 / 65536: the two kernels of k_fft_2p.hip, frame group by frame group
    int group_frames = 0;    // ... frames per group (the batch set's scratch holds one group's intermediate of every band)
    int reserve_cus = 0;     // k_fft_r32: CUs its grid leaves to the other streams' kernels (fft_reserve_cus; 0 for every other kernel)
    bool reserve_forced = false;  // ... as SDR_FFT_RESERVE gave it (the launcher caps the rule's value at kReserveDeviceShare of the device, not a forced one)
    InFormat fmt = InFormat::F32;  // what the kernel reads
    bool windowed = false;         // the windowed form of the kernel (the bank has a window: sdr_set_window)
    bool strided = false;          // frames start every hop < N samples (host/overlap.h); k_fft_r32 has a kernel of its own for that
    int frames_per_wg = 0;  // the 16-point kernels: frames per workgroup (fft_frames_per_wg; 1 for sc16 and 8-bit input); 0 for k_fft_r32 and k_fft_2p
};

// N = 32768 and 65536 (k_fft_2p.hip): frames per group of the two phases.  A group's float64 intermediate is 16 bytes per
// sample of every band.  Groups that fit the 256 MiB Infinity Cache were the first design; measured, phase B does not gain
// from them (0.99 ms per 4096-frame batch of 32768 points in 64 MiB groups, 0.92 ms as one whole-batch group) and every
// group costs two launches, so a group is 128 MiB: within 3 % of whole batches at an eighth of their scratch.
constexpr int kFft2pGroupMiB = 128;  // measured end to end: 64 MiB groups 67, 128 MiB 74, whole batches 76 GS/s
// frames per group of a bank of n_bands bands of N = n whose batches hold at most max_frames frames (0 below N = 32768)
inline int fft2p_group_frames(const Switches &sw, int n, int n_bands, int max_frames)
{
    if (n <= 16384 || n_bands <= 0 || max_frames <= 0)
        return 0;
    const int mib = sw.fft2p_group_mb >= 0 ? sw.fft2p_group_mb : kFft2pGroupMiB;
    const long per_frame = (long)n_bands * n * 16;
    const long f = mib == 0 ? max_frames : ((long)mib << 20) / per_frame;
    return (int)(f < 1 ? 1 : (f > max_frames ? max_frames : f));
}

// The 16-point kernels' float32 form (k_fft_psd<LOGN, MULTI, WIN...>, plain and windowed) can give a workgroup several consecutive frames.
// frames per workgroup when the plan asks for none (FftChoice::fpw, SDR_FFT_FPW)
constexpr int kDefaultFpw = 1;  // in the pipeline short-lived workgroups win: 0.250 (1) / 0.253 (2) / 0.291 (4) / 0.294 ms (8) per step, standalone the other way round (0.174 / 0.166 / 0.165 / 0.164 ms)
// a workgroup's frames are consecutive; never fewer workgroups than CUs can take (a short batch keeps one
// frame per workgroup)
inline int fft_frames_per_wg(int fpw_asked, int n_frames, int n_bands)
{
    int fpw = fpw_asked > 0 ? fpw_asked : kDefaultFpw;
    while (fpw > 1 && (long)((n_frames + fpw - 1) / fpw) * n_bands < 256)
        fpw /= 2;
    return fpw;
}

// N = 16384 has two kernels: k_fft_psd.h's 16-point one and k_fft_r32.h (512 threads x 32 points, the next frame
// prefetched into registers), whose workgroups - one per CU - claim frames from a counter.  By default the 32-point kernel
// runs from 1024 frames per launch on (measured by batch size) and while the listener slots fit its tap (one per thread).
// sc16 input takes the same choice (k_fft_r32<InSc16, .> or k_fft_psd_narrow<InSc16, 14, .>): the rule does not look at the format.
// (bench.py restates the frame-count rule to name the kernel in its report.)
// windowed: the bank has a window (sdr_set_window).  k_fft_r32 has no windowed form - it has no register left for a
// thread's 32 window values beside its prefetched frame - so a windowed batch never takes it, SDR_FFT_R32=1 or not: N =
// 16384 runs the 16-point kernel at every batch length, and k_cum_refine reads psd columns (no wide tap).
// fmt, hop: the input format and the samples from one frame's start to the next (0 or n: dense frames).
// What the launchers once refused at run time cannot be planned: k_fft_r32 with a window or at n != 16384, the two-phase
// kernels at n <= 16384, a windowed 8-bit batch on the float32 / sc16 unit (tests/host/test_fft_kernel_choice.cpp).
inline FftChoice fft_choice(const Switches &sw, int n, int n_frames, int n_bands, int tap_n, bool windowed = false, InFormat fmt = InFormat::F32,
                            int hop = 0)
{
    FftChoice c;
    c.r32 = !windowed && n == 16384 && tap_n <= kR32MaxTap && (sw.fft_r32 == 1 || (sw.fft_r32 < 0 && (long)n_frames * n_bands >= 1024));
    c.fpw = sw.fft_fpw;
    c.wide_tap = c.r32 && tap_n > 0;  // (never at N > 16384: k_cum_refine reads psd columns there)
    c.two_phase = n > 16384;
    c.fmt = fmt;
    c.windowed = windowed;
    c.strided = hop != 0 && hop != n;
    // sc16 and 8-bit input: one frame per workgroup, always (the multi-frame workgroup is float32-only)
    c.frames_per_wg = c.r32 || c.two_phase ? 0 : fmt != InFormat::F32 ? 1 : fft_frames_per_wg(sw.fft_fpw, n_frames, n_bands);
    return c;
}

// One id per kernel symbol a batch can launch first (the two-phase ids name phase A; k_fft2p_b follows every one of them).
enum class FftKernel {
    // k_fft_psd.h, instantiated by k_fft_psd.hip, k_fft_psd_win.hip and k_fft_psd_iq8.hip (PSD_IQ8*: cs8 and cu8, a launch argument)
    PSD, PSD_MULTI, PSD_SC16, PSD_IQ8, PSD_WIN, PSD_WIN_MULTI, PSD_SC16_WIN, PSD_IQ8_WIN,
    // k_fft_r32.h, one instance per k_fft_r32*.hip unit (R32*_IQ8: cs8 and cu8, a launch argument)
    R32, R32_SC16, R32_IQ8, R32_HOP, R32_HOP_SC16, R32_HOP_IQ8,
    // k_fft_2p_a.h: phase A's instances, in k_fft_2p.hip (F32, SC16) and k_fft_2p_iq8.hip (CS8, CU8)
    A2P_F32, A2P_SC16, A2P_CS8, A2P_CU8, A2P_WIN_F32, A2P_WIN_SC16, A2P_WIN_CS8, A2P_WIN_CU8,
    COUNT
};

inline FftKernel fft_kernel(const FftChoice &c)
{
    using K = FftKernel;
    const bool iq8 = is_iq8(c.fmt), sc16 = c.fmt == InFormat::SC16;
    if (c.two_phase) {
        switch (c.fmt) {
        case InFormat::F32: return c.windowed ? K::A2P_WIN_F32 : K::A2P_F32;
        case InFormat::SC16: return c.windowed ? K::A2P_WIN_SC16 : K::A2P_SC16;
        case InFormat::CS8: return c.windowed ? K::A2P_WIN_CS8 : K::A2P_CS8;
        default: return c.windowed ? K::A2P_WIN_CU8 : K::A2P_CU8;
        }
    }
    if (c.r32) {
        if (c.strided)
            return iq8 ? K::R32_HOP_IQ8 : sc16 ? K::R32_HOP_SC16 : K::R32_HOP;
        return iq8 ? K::R32_IQ8 : sc16 ? K::R32_SC16 : K::R32;
    }
    if (iq8)
        return c.windowed ? K::PSD_IQ8_WIN : K::PSD_IQ8;
    if (sc16)
        return c.windowed ? K::PSD_SC16_WIN : K::PSD_SC16;
    if (c.frames_per_wg > 1)
        return c.windowed ? K::PSD_WIN_MULTI : K::PSD_MULTI;
    return c.windowed ? K::PSD_WIN : K::PSD;
}

// The kernel's label: what tests and tools read through the plan, and the symbol's base name in the resource listings taken
// while each kernel had a name of its own (profiles/*_kernel_resources.txt).  The k_fft_r32, k_fft_psd and k_fft2p_a
// kernels are template instances now; their labels stay.
inline const char *fft_kernel_name(FftKernel k)
{
    using K = FftKernel;
    switch (k) {
    case K::PSD: case K::PSD_MULTI: return "k_fft_psd";
    case K::PSD_SC16: return "k_fft_psd_sc16";
    case K::PSD_IQ8: case K::PSD_IQ8_WIN: return "k_fft_psd_iq8";
    case K::PSD_WIN: case K::PSD_WIN_MULTI: return "k_fft_psd_win";
    case K::PSD_SC16_WIN: return "k_fft_psd_sc16_win";
    case K::R32: return "k_fft_r32";
    case K::R32_SC16: return "k_fft_r32_sc16";
    case K::R32_IQ8: return "k_fft_r32_iq8";
    case K::R32_HOP: return "k_fft_r32_hop";
    case K::R32_HOP_SC16: return "k_fft_r32_hop_sc16";
    case K::R32_HOP_IQ8: return "k_fft_r32_hop_iq8";
    case K::A2P_F32: case K::A2P_SC16: case K::A2P_CS8: case K::A2P_CU8: return "k_fft2p_a";
    case K::A2P_WIN_F32: case K::A2P_WIN_SC16: case K::A2P_WIN_CS8: case K::A2P_WIN_CU8: return "k_fft2p_win_a";
    case K::COUNT: break;
    }
    return "";
}

// k_fft_r32's grid is one persistent workgroup per CU: 254 VGPRs at two waves per SIMD and about 160 KB of LDS, so nothing
// else fits on a CU it holds, and it holds it until the launch ends.  With every CU taken, the other streams' kernels - the
// scan, then the chain of thresholds, gather, decode, cumulate, refine, find-peaks and the pack kernels - find a CU only
// between two FFT launches, one dependent stage per boundary: a batch's latency grows until every set of the ring is in
// flight, the caller waits for a set, and the FFT queue idles 0.21 - 0.23 ms of a 0.72 ms config-3 step.  So the grid
// leaves CUs free: enough for the scan's workgroups (each holds a whole CU: 115 KB of LDS) in kReserveRounds rounds, plus
// kReserveExtra for the chain kernels (k_cum_refine's 1024-thread workgroups among them), at most kReserveMax - a quarter
// of the 256-CU device the rule was measured on; on a smaller device or a partition the launcher caps the rule's value at
// CUs / kReserveDeviceShare.  The FFT launch grows by CUs / (CUs - reserve), the launches follow each other 6 - 8 us apart
// and the step is the launch.  Measured on one MI355X, GS/s of the 2000-step line, one band, 256 listeners, by reserve
// forced with SDR_FFT_RESERVE, ONE run per figure (profiles/reserve_sweep.jsonl; HISTORY has the 20-step line and a
// second box).  This box's other runs at reserve 0 gave 201.5 - 202.7, so read the row against 194 - 203, not 194:
//   8192 frames   0: 194   48: 205   56: 210   60: 212   64: 220   68: 218   72: 216   80: 211
//   4096 frames   0: 178   32: 197   48: 194   64: 210   72: 210
//   2048 frames   0: 159   16: 162   32: 183   43: 182   64: 185
// Interleaved pairs against the parent commit, the figure to quote: 1.09 (2000 steps), 1.11 (20 steps) at 8192 frames
// (profiles/reserve_bench_pairs.json).  64 wins at 8192 frames and loses nowhere; between 60 and 64 the gain doubles (64
// free CUs are eight on each of the eight XCDs), so the constants put every batch of 4096 frames and more at the clamp:
// 82 - 84 scan workgroups / 2 + 24 > 64.  Every measurement is one band with 256 listeners: batches of several bands on
// k_fft_r32 (24 bands: 48 or 64 CUs by the same formula) and banks with few listeners take the rule unmeasured.
// The reserve helps only where the other stages can run BESIDE an FFT launch: the runtime deals its hardware queues to
// streams as it likes, and where the FFT's stream (the caller's) shares a queue with one of the bank's streams the
// launches only get longer - 0.91 of the parent commit in those runs of tools/sc16_rate.py.  The bank probes that
// (sdr_bank::fft_queue_alone, capi_bank.hip probe_fft_queue) and the rule reserves nothing on a shared queue.
// No reserve where the batch does not run k_fft_r32, where the chains compute the noise floor (their many small workgroups
// are not what the rule was measured with), and below kReserveMinFrames frames per launch, the shortest batch measured.
// scan_wgs: workgroups of k_psd_scan (n_slots x scan_parts x n_bands).  SDR_FFT_RESERVE=k forces k CUs for every k_fft_r32
// launch (the launcher keeps at least one workgroup).
constexpr int kReserveRounds = 2;
constexpr int kReserveExtra = 24;
constexpr int kReserveMax = 64;
constexpr int kReserveDeviceShare = 4;  // the launcher caps the rule's value at CUs / 4 (a forced one it takes as it is)
constexpr int kReserveMinFrames = 2048;
inline int fft_reserve_cus(const Switches &sw, const FftChoice &c, bool noise_scan, int n_frames, int n_bands, int scan_wgs, bool fft_queue_alone = true)
{
    if (!c.r32)
        return 0;
    if (sw.fft_reserve >= 0)
        return sw.fft_reserve;
    if (!noise_scan || !fft_queue_alone || (long)n_frames * n_bands < kReserveMinFrames)
        return 0;
    const int r = (scan_wgs + kReserveRounds - 1) / kReserveRounds + kReserveExtra;
    return r > kReserveMax ? kReserveMax : r;
}

enum class Refine { NONE, NARROW, WIDE };

struct BatchGeometry {
    int n_bands, n, max_batch_frames, max_chunks;
    // the FFT's stream was found on a hardware queue that none of the bank's other streams uses (sdr_bank::fft_queue_alone,
    // probed at sdr_create and sdr_set_stream): only then can the other stages run beside an FFT launch
    bool fft_queue_alone = true;
};

struct BatchPlan {
    int stream[K_COUNT];  // Stage of each KernelId
    FftChoice fft;
    bool noise_scan;   // k_psd_scan (else the chains: k_window_means -> k_noise_stats)
    int force_exact;   // k_psd_scan's literal fallback (tests)
    bool var_mfma;     // the chains' variance kernel: the matrix pipe (else two vector-ALU chain groups per workgroup)
    int wm_wpb;        // the chains' window sums: windows per workgroup (0: launch_window_means' rule)
    bool bound;        // the completed cumulations are bounded, and refined where FindPeaks looks (else every slot exact)
    bool bound_done;   // ... and k_psd_scan forms the bound's unit counts (k_bound_finish finishes them)
    int scan_parts;    // workgroups a slot's frames are dealt over by k_psd_scan; k_bound_finish adds as many partial counts
    int n_slots;       // cumulation slots the batch touches: grid of k_psd_scan and k_cumulate
    int n_chunks;      // cumulations the batch completes
    int new_count;     // cumulationCount after the batch
    Refine refine;     // the refinement's workgroup shape (NONE: no bound)
    // sdr_enable_rows: k_cum_rows reduces every completed cumulation to row_columns values, on rows_stream behind the
    // cumulate step (the find-peaks stage's stream: its event, which sdr_poll looks at, follows).  Off: no launch at all.
    bool rows;
    int rows_stream;
    // sdr_enable_reports: k_report_marks in front of the decoder and k_listen_report behind it, both on reports_stream
    // (the decode stage's stream: its event, which sdr_poll looks at, follows the pack kernel behind them).  Only where the
    // batch has listener slots; off: no launch at all.
    bool reports;
    int reports_stream;
};

// One batch of n_frames frames that starts at cumulationCount count0, max_slots listener slots in use.  capturing: the
// batch is being recorded into a graph (sdr_graph_capture), replayed later at whatever count0 and without stream changes.
// windowed: the bank has a window (fft_choice).  row_columns: sdr_enable_rows' setting (0: rows off).  reports:
// sdr_enable_reports' setting.  fmt, hop: the batch's input format and frame stride (fft_choice).
inline BatchPlan plan_batch(const Switches &sw, const BatchGeometry &g, int n_frames, int count0, bool capturing, int max_slots,
                            bool windowed = false, int row_columns = 0, bool reports = false, InFormat fmt = InFormat::F32, int hop = 0)
{
    BatchPlan p;
    // Which of the bank's four streams each kernel runs on.  The step is as long as the longest stream, and kernels that
    // carry state from batch to batch (thresholds, decode, cumulate) must keep their stream so that the stream orders the
    // batches.
    const int plan[K_COUNT] = {/* fft */ S_FFT,        /* window means */ S_NOISE, /* noise stats */ S_NOISE, /* thresholds */ S_PEAKS,
                               /* gather */ S_LISTEN,  /* cumulate */ S_PEAKS,     /* find peaks */ S_PEAKS,  /* decode */ S_LISTEN};
    for (int k = 0; k < K_COUNT; k++)
        p.stream[k] = plan[k];
    // Small geometries (one band of N <= 8192, two of 4096 ...): the FFT of a batch is shorter than its decoders, whose time
    // goes with the frames, not the samples - the listen stream is the longest, and the gather, which carries no state
    // from batch to batch and so may run on any stream, moves behind the thresholds it waits for anyway (config 2:
    // 0.206 -> 0.142 ms per 4096-frame step, 80 -> 118 GS/s; config 3 unchanged within a percent either way, config 5's
    // share 10 % SLOWER with it: its peaks stream is the full one).  Not under capture: a replay's graphs are cut by stream.
    if (!capturing && (long)g.n_bands * g.n <= 8192)
        p.stream[K_LISTEN_GATHER] = S_PEAKS;
    for (int k = 0; k < K_COUNT; k++)
        if (sw.diag_plan[k] >= 0)
            p.stream[k] = sw.diag_plan[k];

    p.fft = fft_choice(sw, g.n, n_frames, g.n_bands, max_slots, windowed, fmt, hop);
    p.fft.group_frames = fft2p_group_frames(sw, g.n, g.n_bands, g.max_batch_frames);

    // noise floor: the one-pass scan unless the chains are asked for or the windows are too wide for it (noise_scan_at)
    p.noise_scan = noise_scan_at(sw, g.n);
    p.force_exact = sw.force_exact;
    // the chains' variance: two vector-ALU chain groups per workgroup for long batches (less CU time), the matrix-pipe
    // kernel for short ones (less latency) - see k_noise.hip NS_GROUPS_VALU; never by default above N = 16384 (var_mfma_at)
    p.var_mfma = var_mfma_at(sw, g.n, n_frames);
    p.wm_wpb = sw.wm_wpb;

    // Bound-and-refine replaces the exact kernel's work with three launches on the peaks stream; on a short batch their fixed
    // latencies (a refinement is a chain of a hundred scattered sector reads per candidate, whatever the batch) make that
    // stream the longest of the four: config 3 at 2048 frames per batch 135-143 GS/s against 150 with every slot exact.  From
    // 64 M samples per batch on it pays (config 3 at 8192 frames, config 5's share of 8 x 2048 x 8192).
    p.bound = sw.cum_bound >= 0 ? sw.cum_bound != 0 : (double)n_frames * (double)g.n_bands * (double)g.n >= 64.0 * 1024.0 * 1024.0;
    p.bound_done = p.noise_scan && p.bound;

    // cumulations: the batch completes n_chunks and touches one more slot when it leaves one open.  A captured batch is
    // replayed at any cumulationCount: its grids cover the most chunks a batch of this length can complete, plus the open one.
    p.n_chunks = (count0 + n_frames) / SDR_CUMULATION_SIZE;
    p.new_count = (count0 + n_frames) % SDR_CUMULATION_SIZE;
    p.n_slots = p.n_chunks + (p.new_count != 0 ? 1 : 0);
    if (capturing) {
        p.n_chunks = (SDR_CUMULATION_SIZE - 1 + n_frames) / SDR_CUMULATION_SIZE;
        p.n_slots = p.n_chunks + 1;
    }
    // two parts while the slots alone are fewer than a quarter of the CUs; from there on whole slots: with 16-byte loads a
    // workgroup walks a frame in 1.6 us, and 83 fat workgroups hold less CU time than 166 - config 3: 205.5 -> 209.7 GS/s.
    // Measured again beside the FFT grid's reserve (64 free CUs): two parts at every batch length 220.9 / 220.9 GS/s, this
    // rule 221.7 / 220.4 - no difference, the rule stays (profiles/reserve_plan_rules.jsonl)
    p.scan_parts = (long)p.n_slots * g.n_bands < 64 ? 2 : 1;
    p.fft.reserve_cus = fft_reserve_cus(sw, p.fft, p.noise_scan, n_frames, g.n_bands, p.n_slots * p.scan_parts * g.n_bands, g.fft_queue_alone);
    p.fft.reserve_forced = p.fft.r32 && sw.fft_reserve >= 0;

    // Spans of 4096 bins x 256 threads keep a cumulation's refinement - a latency chain of a hundred scattered sector reads -
    // short where the peaks stream's length bounds the step (few cumulations per batch).  With many cumulations per batch
    // what counts is the CU time the kernel HOLDS: four waves of a small workgroup hold a whole CU against the FFT's
    // workgroups just as sixteen do, so a workgroup takes the whole row (10.9 -> CU-ms per 8192-frame step).  With CUs
    // left free beside the FFT (fft_reserve_cus) that reason is gone, and so is the difference: SDR_REFINE_WIDE=0 220.9 /
    // 221.1 GS/s against 221.7 / 220.4 with the whole row at config 3 - the rule stays (profiles/reserve_plan_rules.jsonl).
    const bool wide = sw.refine_wide >= 0 ? sw.refine_wide != 0 : (g.n >= 4096 && (long)p.n_chunks * g.n_bands >= 64);
    p.refine = !p.bound ? Refine::NONE : wide ? Refine::WIDE : Refine::NARROW;
    // rows only where the batch completes a cumulation (a captured batch may at any replay: n_chunks is its maximum)
    p.rows = row_columns > 0 && p.n_chunks > 0;
    p.rows_stream = p.stream[K_FIND_PEAKS];
    // reports only where the listen stages run (issue_listen leaves them out without a listener slot)
    p.reports = reports && max_slots > 0;
    p.reports_stream = p.stream[K_LISTEN_DECODE];
    return p;
}

// ---- the order of a batch's stages.  The scheduler issues them in this order: FFT, window means, noise stats, thresholds,
// gather, decode, cumulate, find-peaks.  A stage publishes an event (BatchSet::done) whether or not it launches a kernel.

// Who waits for whom, in issue order: stage k starts once stage `dep` of the same batch is done.  The scheduler turns an
// entry into a wait only where the two stages run on different streams (a stream orders its own kernels).
struct StageDep {
    int k, dep;
};
struct StageDeps {
    static constexpr int kMax = 10;
    int n = 0;
    StageDep d[kMax];
};
// peak_scan: the batch runs the peak scan (sdr_set_find_peaks on and the batch completes a cumulation)
inline StageDeps stage_deps(const BatchPlan &p, bool peak_scan)
{
    StageDeps s;
    auto add = [&s](int k, int dep) { s.d[s.n++] = StageDep{k, dep}; };
    add(K_WINDOW_MEANS, K_FFT);
    add(K_NOISE_STATS, K_WINDOW_MEANS);
    add(K_THRESHOLDS, K_NOISE_STATS);
    add(K_LISTEN_GATHER, K_THRESHOLDS);
    add(K_LISTEN_GATHER, K_FFT);
    add(K_LISTEN_DECODE, K_LISTEN_GATHER);
    add(K_CUMULATE, K_FFT);
    if (p.bound_done)  // k_psd_scan wrote the bounds of the completed cumulations: the carry is added to slot 0's by k_bound_finish
        add(K_CUMULATE, K_WINDOW_MEANS);
    add(K_FIND_PEAKS, K_CUMULATE);
    if (peak_scan)  // needs the completing frame's peak threshold
        add(K_FIND_PEAKS, K_THRESHOLDS);
    return s;
}

// Set reuse: the FFT of batch i + RING writes the buffer set that batch i used, once every reader of the set is done.  One
// stage stands for each stream - the last one issued on it, whose event follows all the stream's earlier ones - so the
// FFT's queue gets one wait per other stream, not one per stage.  out[st]: that stage for stream st, -1 where the stream
// runs none of them or is the FFT's own (which orders its batches itself).
inline void set_reuse_stages(const BatchPlan &p, int out[N_STAGES])
{
    static constexpr int issue_order[] = {K_WINDOW_MEANS, K_NOISE_STATS, K_THRESHOLDS, K_LISTEN_GATHER, K_LISTEN_DECODE, K_CUMULATE, K_FIND_PEAKS};
    for (int st = 0; st < N_STAGES; st++)
        out[st] = -1;
    for (int k : issue_order)
        out[p.stream[k]] = k;
    out[p.stream[K_FFT]] = -1;
}

// Graph mode records one graph per stream plus, as a graph of its own in front of the peaks stream's, the thresholds (the
// listen graph starts behind them, not behind the cumulations).  Is kernel k part of graph `graph` (a Stage, or G_THRESHOLDS)?
constexpr int G_THRESHOLDS = N_STAGES, N_GRAPHS = N_STAGES + 1;
inline bool in_graph(const BatchPlan &p, int k, int graph)
{
    return graph == G_THRESHOLDS ? k == K_THRESHOLDS : (k != K_THRESHOLDS && p.stream[k] == graph);
}

}  // namespace sdr
