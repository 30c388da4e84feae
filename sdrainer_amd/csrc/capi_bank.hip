// capi_bank.hip — the bank behind the C ABI (include/sdrainer_hip.h): creation and destruction of its HBM-resident
// state, the control calls that touch state owned by a pipeline stage (attach / detach / setters: applied between
// batches, as the reference applies them between frames, rx/receiver.go:166-172), profiling.  The scheduler is
// capi_process.hip, the host-fed input capi_staged.hip, delivery capi_results.hip, graph mode capi_graph.hip, reads
// capi_read.hip (see bank.h).
#include "bank.h"
#include "chain.h"
#include "twiddles.h"

using namespace sdrcapi;

namespace sdr {
int set_error(int code, const char *msg)  // front.h: what fail and HIP_TRY report through
{
    g_last_error = msg;
    return code;
}

// what an sdr_chain reads of the bank it borrows (chain.h): the geometry and the three states it refuses at creation
ChainBankView chain_bank_view(const sdr_bank *b)
{
    ChainBankView v{};
    v.n_bands = b->cfg.n_bands;
    v.block_size = b->cfg.block_size;
    v.hop = b->hop;
    v.max_batch_frames = b->cfg.max_batch_frames;
    v.device_id = b->cfg.device_id;
    v.stream = b->stream[S_FFT];
    v.graph_captured = b->graph_ready;
    v.defer_listen = b->defer_listen || b->listen_pending;
    for (int band = 0; band < b->cfg.n_bands; band++)
        if (b->in.staged[band].staged != 0 || b->in.staged[band].history != 0 || b->in.staged_kind[band] != sdr::StagedKind::None)
            v.input_staged = true;
    return v;
}
}  // namespace sdr

namespace sdrcapi {
std::unique_ptr<host::DeliveryBackend> make_results_backend(sdr_bank *b);  // capi_results.hip

void resolve_profile(sdr_bank *b)
{
    for (auto &p : b->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.second.first, p.second.second) == hipSuccess) {
            b->prof_ms[p.first] += ms;
            b->prof_n[p.first] += 1;
        }
        (void)hipEventDestroy(p.second.first);
        (void)hipEventDestroy(p.second.second);
    }
    b->pending.clear();
}

int sync_bank(sdr_bank *b)
{
    HIP_TRY(hipSetDevice(b->device));
    {
        const int frc = flush_late_attached(b);  // (whoever synchronises next may read or write slots)
        if (frc)
            return frc;
    }
    for (int s = 0; s < N_STAGES; s++)
        HIP_TRY(hipStreamSynchronize(b->stream[s]));
    b->slots_put = false;
    resolve_profile(b);
    return SDR_OK;
}

// Does the FFT's stream (the caller's) run on a hardware queue that none of the bank's own streams uses?  The runtime deals
// its few hardware queues to streams as they are first used and tells nobody which; kernels of two streams on one queue run
// one after the other, and the CUs k_fft_r32's grid would leave to the tail (host/batch_plan.h fft_reserve_cus) then only
// make its launch longer.  So the bank looks: a kernel that spins for kProbeSpinUs on the FFT's stream, an empty kernel
// on each of its own streams; an empty kernel that ends while the spin still runs was not behind it in its queue.  An
// answer that comes late (the host thread descheduled) reads as "shared", which costs the reserve's gain and nothing else.
// Only banks whose plan could reserve are probed (N = 16384, the stages on streams of their own, no forced reserve).
constexpr int kProbeSpinUs = 300;
__global__ void k_queue_probe_spin(unsigned ticks, unsigned *sink)
{
    // wall_clock64 counts at 100 MHz; the loop is bounded so that it ends whatever the clock does
    const unsigned long long t0 = wall_clock64();
    unsigned n = 0;
    for (int i = 0; i < (1 << 20) && wall_clock64() - t0 < ticks; i++) {
        __builtin_amdgcn_s_sleep(32);
        n++;
    }
    if (n == 0xffffffffu)
        *sink = n;
}
__global__ void k_queue_probe_nop() {}

int probe_fft_queue(sdr_bank *b)
{
    b->fft_queue_alone = true;
    if (b->cfg.block_size != 16384 || b->sw.no_overlap || b->sw.fft_reserve >= 0)
        return SDR_OK;
    HIP_TRY(hipSetDevice(b->device));
    hipEvent_t spin_done = nullptr, nop_done[N_STAGES] = {};
    auto cleanup = [&] {
        if (spin_done)
            (void)hipEventDestroy(spin_done);
        for (hipEvent_t e : nop_done)
            if (e)
                (void)hipEventDestroy(e);
    };
    hipError_t e = hipEventCreateWithFlags(&spin_done, hipEventDisableTiming);
    for (int s = 1; s < N_STAGES && e == hipSuccess; s++)
        e = hipEventCreateWithFlags(&nop_done[s], hipEventDisableTiming);
    // every stream's queue is dealt by now: an empty kernel on each, finished, before the probe proper
    for (int s = 0; s < N_STAGES && e == hipSuccess; s++) {
        hipLaunchKernelGGL(k_queue_probe_nop, dim3(1), dim3(1), 0, b->stream[s]);
        e = hipStreamSynchronize(b->stream[s]);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_queue_probe_spin, dim3(1), dim3(1), 0, b->stream[S_FFT], (unsigned)kProbeSpinUs * 100u, reinterpret_cast<unsigned *>(b->drops.p));
        e = hipEventRecord(spin_done, b->stream[S_FFT]);
    }
    for (int s = 1; s < N_STAGES && e == hipSuccess; s++) {
        hipLaunchKernelGGL(k_queue_probe_nop, dim3(1), dim3(1), 0, b->stream[s]);
        e = hipEventRecord(nop_done[s], b->stream[s]);
    }
    bool shared[N_STAGES] = {};
    for (int s = 1; s < N_STAGES && e == hipSuccess; s++) {
        e = hipEventSynchronize(nop_done[s]);
        // (the spin's event is behind the spin in its queue: done already = the empty kernel waited for the spin, or the answer is late)
        shared[s] = b->stream[s] == b->stream[S_FFT] || hipEventQuery(spin_done) == hipSuccess;
        if (shared[s])
            b->fft_queue_alone = false;
    }
    if (e == hipSuccess)
        e = hipStreamSynchronize(b->stream[S_FFT]);
    cleanup();
    if (e != hipSuccess)
        return fail(SDR_ERR_HIP, std::string("hardware queue probe: ") + hipGetErrorString(e));
    if (b->sw.queue_debug)
        fprintf(stderr, "sdr: FFT stream %s (noise %d listen %d peaks %d share its hardware queue)\n",
                b->fft_queue_alone ? "has a hardware queue to itself" : "SHARES a hardware queue: no CUs reserved", (int)shared[S_NOISE], (int)shared[S_LISTEN],
                (int)shared[S_PEAKS]);
    return SDR_OK;
}

int check_band(sdr_bank *b, int band)
{
    if (!b)
        return fail(SDR_ERR_BAD_ARG, "null bank");
    if (band < 0 || band >= b->cfg.n_bands)
        return fail(SDR_ERR_BAD_ARG, "band out of range");
    return SDR_OK;
}

int check_listener(sdr_bank *b, int band, int lid)
{
    int rc = check_band(b, band);
    if (rc)
        return rc;
    if (lid < 0 || lid >= b->n_slots[band])
        return fail(SDR_ERR_BAD_ARG, "listener id out of range");
    return SDR_OK;
}


// one batch's buffers, stage events and (if bulk delivery is on) its block of pinned host memory
hipError_t alloc_set(sdr_bank *b, BatchSet &S)
{
    const sdr_config &c = b->cfg;
    const size_t B = (size_t)c.n_bands, F = (size_t)c.max_batch_frames, L = (size_t)c.max_listeners, N = (size_t)c.block_size;
    hipError_t e = hipSuccess;
#define SET_ALLOC(buf, count)            \
    do {                                 \
        if (e == hipSuccess)             \
            e = (buf).alloc(count);      \
    } while (0)
    SET_ALLOC(S.psd, B * F * N);
    SET_ALLOC(S.tap, B * F * std::max<size_t>(L, 1));
    if (b->logn == 14) {  // (the kernel that writes them serves this block size only)
        SET_ALLOC(S.tapw, B * F * 4 * std::max<size_t>(L, 1));
        // -1 = no bin: k_fft_r32 rewrites the first min(L, 512) entries per band at every launch; the rest are never
        // written and, zeroed, would claim bin 0 (k_cum_refine reads only the first n_tap <= 512)
        if (e == hipSuccess)
            e = S.tap_used.alloc(B * std::max<size_t>(L, 1), 0xff);
        SET_ALLOC(S.fft_ctr, B * 2);
    }
    // N = 32768 / 65536 (k_fft_2p.hip): one frame group's float64 intermediate of every band.  Per set, so that the FFT
    // launches of replays in flight at the same time (graph mode) never share it.
    SET_ALLOC(S.fft_scratch, B * (size_t)sdr::fft2p_group_frames(b->sw, c.block_size, c.n_bands, c.max_batch_frames) * N);
    SET_ALLOC(S.win_mean, B * F * 10);
    SET_ALLOC(S.recs, B * F);
    SET_ALLOC(S.raw_bits, B * L * (size_t)b->bit_words);
    SET_ALLOC(S.bits, B * L * (size_t)b->bit_words);
    SET_ALLOC(S.edges, B * L * (size_t)b->edge_cap);
    SET_ALLOC(S.edge_counts, B * L);
    SET_ALLOC(S.report_marks, B * L * 2);
    if (c.trace) {
        SET_ALLOC(S.tr_values, B * F * L);
        SET_ALLOC(S.tr_raw, B * F * L);
        SET_ALLOC(S.tr_deb, B * F * L);
        SET_ALLOC(S.slots_before, B * L);
    }
    SET_ALLOC(S.cum_out, B * (size_t)b->max_chunks * N);
    SET_ALLOC(S.cum_part, B * (size_t)b->max_chunks * N);
    SET_ALLOC(S.dev_peaks, B * (size_t)b->max_chunks * (size_t)c.max_peaks);
    SET_ALLOC(S.peak_counts, B * (size_t)b->max_chunks);
#undef SET_ALLOC
#ifndef SDR_STAGE_EVENT_FLAGS
#define SDR_STAGE_EVENT_FLAGS hipEventDisableTiming
#endif
    for (auto &ev : S.done)
        if (e == hipSuccess)
            e = hipEventCreateWithFlags(&ev, SDR_STAGE_EVENT_FLAGS);
    return e;
}

}  // namespace sdrcapi

extern "C" {
#pragma GCC visibility push(default)

const char *sdr_last_error(void) { return g_last_error.c_str(); }
int sdr_abi_version(void) { return SDR_ABI_VERSION; }
const char *sdr_kernel_name(int kernel) { return (kernel >= 0 && kernel < sdr::K_PROFILE_SLOTS) ? kKernelNames[kernel] : ""; }

int sdr_self_check(int device_id)
{
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device_id < 0 || device_id >= ndev)
        return fail(SDR_ERR_BAD_ARG, "device_id out of range");
    int prev_dev = 0;
    HIP_TRY(hipGetDevice(&prev_dev));
    struct Restore {  // (a public entry point: the caller's current device is the caller's)
        int dev;
        ~Restore() { (void)hipSetDevice(dev); }
    } restore{prev_dev};
    HIP_TRY(hipSetDevice(device_id));
    unsigned *d = nullptr, h = 0;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d), sizeof(unsigned)));
    hipError_t e = hipMemset(d, 0, sizeof(unsigned));
    // (tests only: SDR_SELF_CHECK_ORDER=1 / 2 compares against an evaluation order the pipe must not have - the check has to fail)
    const char *ord = getenv("SDR_SELF_CHECK_ORDER");
    if (e == hipSuccess)
        e = sdr::launch_mfma_order_probe(d, ord ? atoi(ord) : 0, nullptr);
    if (e == hipSuccess)
        e = hipMemcpy(&h, d, sizeof h, hipMemcpyDeviceToHost);  // (synchronises with the null stream)
    (void)hipFree(d);
    HIP_TRY(e);
    if (h != 0)
        return fail(SDR_ERR_HIP, "self-check failed: v_mfma_f64_4x4x4 does not add its terms as a sequential, individually rounded chain on this "
                                 "device (" + std::to_string(h) + " of 4096 partial sums differ from the vector ALU's); the variance of "
                                 "FindNoiseFloor would not be bit-exact - this part is not supported");
    return SDR_OK;
}

namespace {
// once per device and process; the verdict is kept (a failing part fails every creation)
static int self_check_once(int device_id)
{
    constexpr int kMax = 64;
    static std::mutex mu;
    static int verdict[kMax];
    static bool done[kMax];
    static std::string message[kMax];
    if (device_id < 0 || device_id >= kMax)
        return sdr_self_check(device_id);
    std::lock_guard<std::mutex> g(mu);
    if (!done[device_id]) {
        verdict[device_id] = sdr_self_check(device_id);
        message[device_id] = g_last_error;
        // only a definite outcome is kept: the probe ran and agreed, or ran and counted mismatches.  A HIP failure on the
        // way (no memory for four bytes, a busy device) says nothing about the silicon: the next creation tries again.
        done[device_id] = verdict[device_id] == SDR_OK || message[device_id].find("self-check failed") != std::string::npos;
    }
    if (verdict[device_id] != SDR_OK)
        g_last_error = message[device_id];
    return verdict[device_id];
}
}  // namespace

int sdr_create(const sdr_config *cfg, sdr_bank **out)
{
    if (!cfg || !out)
        return fail(SDR_ERR_BAD_ARG, "null argument");
    if (cfg->struct_size != (int32_t)sizeof(sdr_config))
        return fail(SDR_ERR_BAD_ARG, "sdr_config.struct_size mismatch (ABI)");
    const int N = cfg->block_size;
    if (N < 512 || N > 65536 || (N & (N - 1)))
        return fail(SDR_ERR_BAD_SIZE, "block_size must be a power of two in [512, 65536]");
    if (cfg->n_bands < 1 || cfg->sample_rate < 1 || cfg->max_batch_frames < 1 || cfg->max_listeners < 0 ||
        cfg->max_peaks < 1)
        return fail(SDR_ERR_BAD_ARG, "non-positive geometry");
    if (cfg->edge_width < 0 || N - 2 * cfg->edge_width < 10)
        return fail(SDR_ERR_BAD_ARG, "edge_width leaves fewer than 10 bins: the reference's windowSize would be 0 (NaN)");
    if (!sdr::hop_valid(cfg->hop, N))
        return fail(SDR_ERR_BAD_ARG, "hop must be 0 (= block_size) or a power of two with block_size / 16 <= hop <= block_size and hop >= 32");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (cfg->device_id < 0 || cfg->device_id >= ndev)
        return fail(SDR_ERR_BAD_ARG, "device_id out of range");
    HIP_TRY(hipSetDevice(cfg->device_id));

    sdr_bank *b = new sdr_bank();
    b->cfg = *cfg;
    b->hop = sdr::effective_hop(cfg->hop, N);
    b->sw = sdr::read_switches();
    b->device = cfg->device_id;
    b->logn = ilog2(N);
    b->edge_width = cfg->edge_width;
    b->find_peaks = cfg->find_peaks;
    const size_t B = (size_t)cfg->n_bands, L = (size_t)cfg->max_listeners;
    b->max_chunks = cfg->max_batch_frames / SDR_CUMULATION_SIZE + 2;
    b->edge_cap = cfg->max_batch_frames < 8192 ? cfg->max_batch_frames : 8192;
    b->bit_words = (cfg->max_batch_frames + 63) / 64;

#define ALLOC(buf, count)                                                                              \
    do {                                                                                               \
        hipError_t _e = (buf).alloc(count);                                                            \
        if (_e != hipSuccess) {                                                                        \
            sdr_destroy(b);                                                                            \
            return fail(SDR_ERR_HIP, std::string("hipMalloc " #buf ": ") + hipGetErrorString(_e));     \
        }                                                                                              \
    } while (0)

    // SDR_NO_OVERLAP=1 runs every stage on the caller's stream (kernel-by-kernel profiling)
    for (int s = 1; s < N_STAGES && !b->sw.no_overlap; s++) {
        hipError_t e = hipStreamCreateWithFlags(&b->stream[s], hipStreamNonBlocking);
        if (e != hipSuccess) {
            sdr_destroy(b);
            return fail(SDR_ERR_HIP, "hipStreamCreate failed");
        }
        b->own_stream[s] = true;
    }
    // The matrix pipe adds the way the variance chains need it to (sdr_self_check), checked BEHIND the creation of the
    // bank's streams: HIP deals hardware queues to streams as they come, and a kernel launched before the bank's streams
    // exist took the queue one of them was to get - two of the bank's streams then shared a queue and graph mode, whose
    // replays overlap stream against stream, ran at 101 instead of 156 GS/s (config 3; round 4, found by bisection).
    // Only the chain kernels (SDR_NOISE_PATH=chains) need it: the default noise path (k_noise_scan.hip) does not use the
    // matrix pipe, so a bank on it depends on no undocumented behaviour and is not probed; nor is a bank of N > 16384, whose
    // default chains keep their variance on the vector ALU (host/batch_plan.h var_mfma_at).
    if (sdr::may_use_matrix_pipe(b->sw, N)) {
        const int sc = self_check_once(cfg->device_id);
        if (sc != SDR_OK) {
            sdr_destroy(b);
            return sc;
        }
    }
    // twiddles: go-dsp's table, re-laid-out per register pass
    {
        std::vector<double> wre, wim;
        fft64::radix2_factors(N, wre, wim);
        const size_t ntw = (size_t)sdr::twiddle_count(b->logn);
        std::vector<fft64::cplx> h(ntw);
        sdr::build_twiddles(b->logn, wre.data(), wim.data(), h.data());
        ALLOC(b->tw, h.size());
        hipError_t e = hipMemcpy(b->tw.p, h.data(), h.size() * sizeof(fft64::cplx), hipMemcpyHostToDevice);
        // tables of the certified dB shortcut (they fold log2 N in)
        std::vector<unsigned char> tab(gomath::kDbTabBytes);
        gomath::build_db_tables(b->logn, tab.data());
        ALLOC(b->db_tab, tab.size());
        if (e == hipSuccess)
            e = hipMemcpy(b->db_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            sdr_destroy(b);
            return fail(SDR_ERR_HIP, "twiddle / table upload failed");
        }
    }
    b->res_backend = make_results_backend(b);
    b->results.reset(new host::Delivery(b->res_backend.get(), RING, GRAPH_PHASES * RING));
    b->set.reserve((size_t)RING + (size_t)GRAPH_PHASES * RING);  // (graph mode adds its sets later: no reallocation, references stay valid)
    b->set.resize(RING);
    for (int r = 0; r < RING; r++) {
        const hipError_t se = alloc_set(b, b->set[r]);
        if (se != hipSuccess) {
            sdr_destroy(b);
            return fail(SDR_ERR_HIP, std::string("allocating a batch buffer set: ") + hipGetErrorString(se));
        }
    }
    ALLOC(b->band_state, B);
    ALLOC(b->drops, 1);
    ALLOC(b->cursors, GRAPH_PHASES * RING);
    ALLOC(b->spectrum_row, (size_t)N);
    ALLOC(b->tap_bins, B * std::max<size_t>(L, 1));
    {
        std::vector<int32_t> free_bins(B * std::max<size_t>(L, 1), -1);
        hipError_t he = hipMemcpy(b->tap_bins.p, free_bins.data(), free_bins.size() * sizeof(int32_t), hipMemcpyHostToDevice);
        if (he != hipSuccess) {
            sdr_destroy(b);
            return fail(SDR_ERR_HIP, "tap table upload failed");
        }
    }
    ALLOC(b->slots, B * L);
    ALLOC(b->morse, cw::kMorseTableSize);
    ALLOC(b->text, B * L * (size_t)b->text_cap);
    ALLOC(b->text_frames, B * L * (size_t)b->text_cap);
    ALLOC(b->edge_pos, B * L * (size_t)cfg->max_batch_frames);
    ALLOC(b->carry[0], B * N);
    ALLOC(b->carry[1], B * N);
#undef ALLOC

    std::vector<uint16_t> h_morse(cw::kMorseTableSize);
    cw::build_morse_table(h_morse.data());
    hipError_t e = hipMemcpy(b->morse.p, h_morse.data(), sizeof(uint16_t) * cw::kMorseTableSize, hipMemcpyHostToDevice);
    b->h_band_state.assign(B, sdr::BandState{});
    for (auto &s : b->h_band_state)
        s.peak_threshold = cfg->peak_threshold;
    if (e == hipSuccess)
        e = hipMemcpy(b->band_state.p, b->h_band_state.data(), sizeof(sdr::BandState) * B, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        sdr_destroy(b);
        return fail(SDR_ERR_HIP, "state upload failed");
    }
    b->h_slots.assign(B * L, sdr::ListenerSlot{});
    b->n_slots.assign(B, 0);
    b->center_frequency.assign(B, 0);
    b->in.staged.assign(B, sdr::StreamStage{N, b->hop, 0, 0});
    b->in.staged_kind.assign(B, sdr::StagedKind::None);
    {
        const int prc = probe_fft_queue(b);  // (the null stream's queue against the bank's; sdr_set_stream looks again)
        if (prc) {
            sdr_destroy(b);
            return prc;
        }
    }
    *out = b;
    return SDR_OK;
}

int sdr_destroy(sdr_bank *b)
{
    if (!b)
        return SDR_OK;
    (void)hipSetDevice(b->device);
    for (int s = 0; s < N_STAGES; s++)
        (void)hipStreamSynchronize(b->stream[s]);
    resolve_profile(b);
    drop_graphs(b);
    if (b->slots_put_ev)
        (void)hipEventDestroy(b->slots_put_ev);
    for (auto &ph : b->phase_done)
        for (auto &ev : ph)
            if (ev)
                (void)hipEventDestroy(ev);
    b->tw.release();
    b->drops.release();
    b->cursors.release();
    b->db_tab.release();
    b->tap_bins.release();
    b->window.release();
    b->spectrum_row.release();
    for (auto &S : b->set)
        S.release();
    if (b->results)
        for (int i = 0; i < b->results->n_sets(); i++)
            results_release_set(b, i);
    b->band_state.release();
    b->slots.release();
    b->morse.release();
    b->text.release();
    b->text_frames.release();
    b->edge_pos.release();
    b->carry[0].release();
    b->carry[1].release();
    for (int s = 0; s < N_STAGES; s++)
        if (b->own_stream[s] && b->stream[s])
            (void)hipStreamDestroy(b->stream[s]);
    if (b->in.copy_stream) {
        (void)hipStreamSynchronize(b->in.copy_stream);
        (void)hipStreamDestroy(b->in.copy_stream);
    }
    for (auto &st : b->in.stage) {
        if (st.h_f32)
            (void)hipHostFree(st.h_f32);
        if (st.h_raw)
            (void)hipHostFree(st.h_raw);
        st.d_f32.release();
        st.d_raw.release();
        if (st.uploaded)
            (void)hipEventDestroy(st.uploaded);
        if (st.consumed)
            (void)hipEventDestroy(st.consumed);
    }
    delete b;
    return SDR_OK;
}

int sdr_set_stream(sdr_bank *b, void *hip_stream)
{
    if (!b)
        return fail(SDR_ERR_BAD_ARG, "null bank");
    int rc = sync_bank(b);
    if (rc)
        return rc;
    for (int s = 1; s < N_STAGES; s++)
        if (!b->own_stream[s])
            b->stream[s] = reinterpret_cast<hipStream_t>(hip_stream);  // SDR_NO_OVERLAP: one stream for all
    b->stream[S_FFT] = reinterpret_cast<hipStream_t>(hip_stream);
    return probe_fft_queue(b);
}

int sdr_sync(sdr_bank *b)
{
    if (!b)
        return fail(SDR_ERR_BAD_ARG, "null bank");
    return sync_bank(b);
}

// Control calls touch state owned by a pipeline stage: drain the pipeline first (they are rare, and
// the reference also applies them between frames only, rx/receiver.go:166-172).
int sdr_attach(sdr_bank *b, int band, int bin, int *listener_id)
{
    int rc = check_band(b, band);
    if (rc)
        return rc;
    const sdr_config &c = b->cfg;
    if (bin < 0 || bin >= c.block_size)
        return fail(SDR_ERR_BAD_ARG, "bin out of range");
    // reuse a released slot first, else grow (ListenerPool.BindNext, rx/listener.go:214-229)
    int lid = -1;
    for (int i = 0; i < b->n_slots[band]; i++)
        if (!b->h_slots[(size_t)band * c.max_listeners + i].active) {
            lid = i;
            break;
        }
    if (lid < 0) {
        if (b->n_slots[band] >= c.max_listeners)
            return fail(SDR_ERR_NO_SLOT, "listener pool exhausted");
        lid = b->n_slots[band]++;
    }
    sdr::ListenerSlot &s = b->h_slots[(size_t)band * c.max_listeners + lid];
    memset(&s, 0, sizeof s);
    s.active = 1;
    s.bin = bin;
    cw::debouncer_init(s.deb, c.signal_debounce);          // NewSpectralDemodulator, cw/spectral.go:25-33
    cw::decoder_init(s.dec, c.sample_rate, sdr::effective_hop(c.hop, c.block_size));  // NewDecoder, cw/decode.go:131-147
    cw::decoder_reset(s.dec);                              // Listener.Attach -> demodulator.Reset, listener.go:88
    s.start_frame = s.tapped_from = (uint32_t)b->total_frames;  // listens from the next frame processed
    rc = sync_bank(b);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpy(b->slots.p + (size_t)band * c.max_listeners + lid, &s, sizeof s, hipMemcpyHostToDevice));
    const int32_t tap_bin = bin;
    HIP_TRY(hipMemcpy(b->tap_bins.p + (size_t)band * c.max_listeners + lid, &tap_bin, sizeof tap_bin, hipMemcpyHostToDevice));
    b->attach_gen++;
    if (listener_id)
        *listener_id = lid;
    return SDR_OK;
}

int sdr_detach(sdr_bank *b, int band, int lid)
{
    int rc = check_listener(b, band, lid);
    if (rc)
        return rc;
    sdr::ListenerSlot &s = b->h_slots[(size_t)band * b->cfg.max_listeners + lid];
    if (!s.active)
        return fail(SDR_ERR_STATE, "listener not attached");
    s.active = 0;
    rc = sync_bank(b);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpy(&b->slots.p[(size_t)band * b->cfg.max_listeners + lid].active, &s.active, sizeof(int32_t),
                      hipMemcpyHostToDevice));
    const int32_t free_bin = -1;
    HIP_TRY(hipMemcpy(b->tap_bins.p + (size_t)band * b->cfg.max_listeners + lid, &free_bin, sizeof free_bin,
                      hipMemcpyHostToDevice));
    b->attach_gen++;
    return SDR_OK;
}

int sdr_attach_at(sdr_bank *b, int band, int bin, int64_t start_frame, int *listener_id)
{
    int rc = check_band(b, band);
    if (rc)
        return rc;
    const sdr_config &c = b->cfg;
    if (bin < 0 || bin >= c.block_size)
        return fail(SDR_ERR_BAD_ARG, "bin out of range");
    const int64_t lo = b->listen_pending ? b->pend.first_frame : b->total_frames;
    if (start_frame < lo || start_frame > b->total_frames)
        return fail(SDR_ERR_BAD_ARG, "start_frame must lie in the batch that waits for its listen half (or be the next frame)");
    if (b->graph_ready)
        return fail(SDR_ERR_STATE, "a graph is captured (sdr_graph_release first)");
    HIP_TRY(hipSetDevice(b->device));
    int lid = -1;
    for (int i = 0; i < b->n_slots[band]; i++)
        if (!b->h_slots[(size_t)band * c.max_listeners + i].active) {
            lid = i;
            break;
        }
    if (lid < 0) {
        if (b->n_slots[band] >= c.max_listeners)
            return fail(SDR_ERR_NO_SLOT, "listener pool exhausted");
        lid = b->n_slots[band]++;
    }
    sdr::ListenerSlot &s = b->h_slots[(size_t)band * c.max_listeners + lid];
    memset(&s, 0, sizeof s);
    s.active = 1;
    s.bin = bin;
    cw::debouncer_init(s.deb, c.signal_debounce);
    cw::decoder_init(s.dec, c.sample_rate, sdr::effective_hop(c.hop, c.block_size));
    cw::decoder_reset(s.dec);
    s.start_frame = (uint32_t)start_frame;
    s.tapped_from = (uint32_t)b->total_frames;  // the FFT of every frame before that has run without this listener
    // (reaches the device with the next sdr_process_listen / process call: flush_late_attached)
    b->late_attached.push_back(band * c.max_listeners + lid);
    b->attach_gen++;
    if (listener_id)
        *listener_id = lid;
    return SDR_OK;
}

int sdr_listener_count(sdr_bank *b, int band)
{
    if (check_band(b, band))
        return -1;
    int n = 0;
    for (int i = 0; i < b->n_slots[band]; i++)
        n += b->h_slots[(size_t)band * b->cfg.max_listeners + i].active;
    return n;
}

int sdr_listener_stop(sdr_bank *b, int band, int lid)
{
    int rc = check_listener(b, band, lid);
    if (rc)
        return rc;
    const size_t idx = (size_t)band * b->cfg.max_listeners + lid;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(sdr::launch_listener_stop(b->slots.p + idx, b->morse.p, b->text.p + idx * b->text_cap,
                                      b->text_frames.p + idx * b->text_cap, b->text_cap,
                                      (uint32_t)std::max<int64_t>(b->total_frames - 1, 0), b->drops.p, b->stream[S_LISTEN]));
    return SDR_OK;
}

int sdr_set_peak_threshold(sdr_bank *b, int band, float threshold)
{
    int rc = check_band(b, band);
    if (rc)
        return rc;
    b->h_band_state[band].peak_threshold = threshold;
    rc = sync_bank(b);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpy(&b->band_state.p[band].peak_threshold, &b->h_band_state[band].peak_threshold, sizeof(float),
                      hipMemcpyHostToDevice));
    return SDR_OK;
}

int sdr_set_edge_width(sdr_bank *b, int edge_width)
{
    if (!b)
        return fail(SDR_ERR_BAD_ARG, "null bank");
    if (edge_width < 0 || b->cfg.block_size - 2 * edge_width < 10)
        return fail(SDR_ERR_BAD_ARG, "edge_width leaves fewer than 10 bins");
    b->edge_width = edge_width;  // a launch parameter: picked up by the next batch
    return SDR_OK;
}

// The table is read by the FFT kernels of batches that may still be queued: drain them, then overwrite it.  A captured
// graph holds the table's pointer and the kernels the plan picked with or without a window, hence SDR_ERR_STATE there.
int sdr_set_window(sdr_bank *b, const float *window, int n)
{
    if (!b)
        return fail(SDR_ERR_BAD_ARG, "null bank");
    if (!window && n != 0)
        return fail(SDR_ERR_BAD_ARG, "null window table with n != 0 (NULL, 0 removes the window)");
    if (window && n != b->cfg.block_size)
        return fail(SDR_ERR_BAD_ARG, "the window table must hold block_size values");
    if (b->listen_pending)
        return fail(SDR_ERR_STATE, "the listen half of a deferred batch is pending (sdr_process_listen first)");
    if (b->graph_ready)
        return fail(SDR_ERR_STATE, "a graph is captured (sdr_graph_release first; set the window, then capture)");
    const int rc = sync_bank(b);
    if (rc)
        return rc;
    if (!window) {
        b->windowed = false;
        return SDR_OK;
    }
    if (!b->window.p)
        HIP_TRY(b->window.alloc((size_t)n));
    std::vector<float> image((size_t)n);  // the values in the order the bank's FFT kernel reads them
    sdr::window_layout(b->logn, window, image.data());
    HIP_TRY(hipMemcpy(b->window.p, image.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    b->windowed = true;
    return SDR_OK;
}

int sdr_set_signal_debounce(sdr_bank *b, int band, int debounce)
{
    int rc = check_band(b, band);
    if (rc)
        return rc;
    // The kernel runs on the listen stream, where the pending half's decoders have not run yet: it would reach frames that
    // lie before the call (the reference applies a control between two frames, rx/receiver.go:217-253).
    if (b->listen_pending)
        return fail(SDR_ERR_STATE, "the listen half of a deferred batch is pending (sdr_process_listen first)");
    if (b->n_slots[band] == 0)
        return SDR_OK;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(sdr::launch_set_debounce(b->slots.p + (size_t)band * b->cfg.max_listeners, b->n_slots[band], debounce,
                                     b->stream[S_LISTEN]));
    return SDR_OK;
}

int sdr_set_center_frequency(sdr_bank *b, int band, int64_t frequency)
{
    int rc = check_band(b, band);
    if (rc)
        return rc;
    std::lock_guard<std::mutex> guard(b->center_mu);  // (a batch takes its snapshot under it)
    b->center_frequency[band] = frequency;
    return SDR_OK;
}

int sdr_set_find_peaks(sdr_bank *b, int on)
{
    if (!b)
        return fail(SDR_ERR_BAD_ARG, "null bank");
    b->find_peaks = on ? 1 : 0;
    return SDR_OK;
}

int sdr_last_batch_frames(sdr_bank *b) { return b ? b->last_frames : -1; }
int64_t sdr_total_frames(sdr_bank *b) { return b ? b->total_frames : -1; }
int sdr_last_batch_chunks(sdr_bank *b) { return b ? b->last_chunks : -1; }

// Only total_frames changes: every 32-bit frame word (the slots' start_frame and tapped_from, the batches' frame_base)
// is cut from it when a listener is attached or a batch is enqueued, and cum_count stays 0 - hence a multiple of the
// cumulation size, so that cumulations still complete at frames = 99 (mod 100).
int sdr_set_first_frame(sdr_bank *b, int64_t frame)
{
    if (!b)
        return fail(SDR_ERR_BAD_ARG, "null bank");
    if (frame < 0 || frame % SDR_CUMULATION_SIZE != 0)
        return fail(SDR_ERR_BAD_ARG, "the first frame must be >= 0 and a multiple of SDR_CUMULATION_SIZE");
    if (b->batch_index != 0 || b->listen_pending)
        return fail(SDR_ERR_STATE, "the bank has processed frames already");
    if (b->graph_ready)
        return fail(SDR_ERR_STATE, "a graph is captured (sdr_graph_release first)");
    for (int band = 0; band < b->cfg.n_bands; band++) {
        if (b->n_slots[band] != 0)
            return fail(SDR_ERR_STATE, "a listener is attached already (set the first frame before the first attach)");
        if (b->in.staged[band].staged != 0 || b->in.staged[band].history != 0 || b->in.staged_kind[band] != sdr::StagedKind::None)
            return fail(SDR_ERR_STATE, "input is staged already (set the first frame before the first push)");
    }
    b->total_frames = frame;
    return SDR_OK;
}

int sdr_profile_enable(sdr_bank *b, int on)
{
    if (!b)
        return fail(SDR_ERR_BAD_ARG, "null bank");
    int rc = sync_bank(b);
    if (rc)
        return rc;
    b->profiling = on != 0;
    return SDR_OK;
}

int sdr_profile_read(sdr_bank *b, int kernel, double *total_ms, int *launches)
{
    if (!b || kernel < 0 || kernel >= sdr::K_PROFILE_SLOTS)
        return fail(SDR_ERR_BAD_ARG, "bad kernel id");
    int rc = sync_bank(b);
    if (rc)
        return rc;
    if (total_ms)
        *total_ms = b->prof_ms[kernel];
    if (launches)
        *launches = b->prof_n[kernel];
    return SDR_OK;
}

int sdr_profile_reset(sdr_bank *b)
{
    if (!b)
        return fail(SDR_ERR_BAD_ARG, "null bank");
    int rc = sync_bank(b);
    if (rc)
        return rc;
    for (int i = 0; i < sdr::K_PROFILE_SLOTS; i++) {
        b->prof_ms[i] = 0;
        b->prof_n[i] = 0;
    }
    return SDR_OK;
}

#pragma GCC visibility pop
}  // extern "C"
