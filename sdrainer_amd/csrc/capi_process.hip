// capi_process.hip — the scheduler of libsdrainer_hip.so: one batch's kernels over the bank's four streams.
//
// The FFT kernel is throughput work that fills the whole chip; everything after it is a set of short, strictly ordered
// chains (float64 noise-floor sums, the rolling means, the per-signal decoders) that occupy a handful of CUs for a long
// time.  Run back to back they would leave the chip idle most of the step, so a bank is a software pipeline over four
// streams (four is also the number of hardware queues HIP maps streams to by default; more streams alias and serialise):
//
//   fft     k_fft_psd(i)                                          (the caller's stream)
//   noise   k_window_means(i) -> k_noise_stats(i)
//   peaks   k_thresholds(i) -> k_cum_bound(i), k_cumulate(i) -> k_find_peaks(i) (-> k_pack_peaks(i))
//   listen  k_listen_gather(i) -> (k_report_marks(i) ->) k_listen_decode(i) (-> k_listen_report(i)) (-> k_pack_listen(i))
//
// Batch i's per-batch buffers (psd, tap, frame records, keying bits, peaks ...) live in set i % RING, and one event per
// stage orders the stages across streams.  Which stream a stage runs on, who waits for whom, which stage stands for its
// stream when fft(i) waits for every reader of set i % RING from batch i - RING, and which graph a kernel belongs to under
// capture are the plan's (host/batch_plan.h: plan_batch, stage_deps, set_reuse_stages, in_graph); this file applies them.
// State that is carried from frame to frame is only ever touched by one kernel, whose stream keeps it in batch order.
// Results leave the device in bulk (capi_results.hip) or are read after sdr_sync(), which drains every stream
// (capi_read.hip).
//
// process_device_body enqueues every batch: it prepares a BatchIssue (the bank, the batch's buffer set and plan, whether
// and for which graph a capture is recording) and runs the parts asked for - the spectral half (issue_spectra), the listen
// half (issue_listen), cumulation and peaks (issue_cumulation) - then commits the host's state (commit_batch).
// BatchIssue::stage is the one place that launches a stage's kernel and publishes its event: the event is an argument of
// the launcher (sdr::LaunchAt, sdr_device.h), which attaches it to its last kernel.
//
// The same body is driven three more ways: recorded into graphs (capi_graph.hip: capture_k / capture_stage), as the
// deferred listen half (sdr_defer_listen ...: the spectral stages of a batch first, listeners bound to frames inside it,
// then the listen stages) and by the staged host input (capi_staged.hip, through process_device_impl).  The file ends
// with the entry points for input that is on the device already and the deferred-listen calls.
#include <string>

#include "bank.h"

using namespace sdrcapi;

namespace sdrcapi {

// sdr_attach_at: the new listener's slot and tap bin reach the device as kernel arguments, in stream order, without a
// synchronous copy (the pipeline keeps running while the host binds listeners)
constexpr int PUT_SLOTS = 16, PUT_BINS = 128;  // per launch (kernel arguments: 16 slots are about 2.5 KB)
struct SlotPack {
    int32_t n;
    int32_t index[PUT_SLOTS];
    sdr::ListenerSlot slot[PUT_SLOTS];
};
struct BinPack {
    int32_t n;
    int32_t index[PUT_BINS], bin[PUT_BINS];
};
__global__ void k_put_slots(sdr::ListenerSlot *slots, SlotPack p)
{
    // (word-wise: a slot is a few dozen words)
    constexpr int W = sizeof(sdr::ListenerSlot) / 4;
    static_assert(sizeof(sdr::ListenerSlot) % 4 == 0, "word copy");
    for (int i = threadIdx.x; i < p.n * W; i += blockDim.x)
        reinterpret_cast<uint32_t *>(slots + p.index[i / W])[i % W] = reinterpret_cast<const uint32_t *>(&p.slot[i / W])[i % W];
}
__global__ void k_put_bins(int32_t *bins, BinPack p)
{
    for (int i = threadIdx.x; i < p.n; i += blockDim.x)
        bins[p.index[i]] = p.bin[i];
}

// The listeners bound by sdr_attach_at since the last flush, to the device: their slots on the listen stream (where the
// decoder, which carries their state, runs; a gather on another stream waits for slots_put_ev - issue_listen),
// their tap bins on the FFT stream (read by the next FFT) - a handful of launches whatever their
// number, and no synchronous copy.
int flush_late_attached(sdr_bank *b)
{
    if (b->late_attached.empty())
        return SDR_OK;
    const std::vector<int> &v = b->late_attached;
    for (size_t at = 0; at < v.size(); at += PUT_SLOTS) {
        SlotPack p{};
        p.n = (int32_t)std::min<size_t>(PUT_SLOTS, v.size() - at);
        for (int i = 0; i < p.n; i++) {
            p.index[i] = v[at + i];
            p.slot[i] = b->h_slots[(size_t)v[at + i]];
        }
        hipLaunchKernelGGL(k_put_slots, dim3(1), dim3(256), 0, b->stream[S_LISTEN], b->slots.p, p);
        HIP_TRY(hipGetLastError());
    }
    if (!b->slots_put_ev)
        HIP_TRY(hipEventCreateWithFlags(&b->slots_put_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(b->slots_put_ev, b->stream[S_LISTEN]));  // (behind every earlier put too: one stream)
    b->slots_put = true;
    for (size_t at = 0; at < v.size(); at += PUT_BINS) {
        BinPack p{};
        p.n = (int32_t)std::min<size_t>(PUT_BINS, v.size() - at);
        for (int i = 0; i < p.n; i++) {
            p.index[i] = v[at + i];
            p.bin[i] = b->h_slots[(size_t)v[at + i]].bin;
        }
        hipLaunchKernelGGL(k_put_bins, dim3(1), dim3(128), 0, b->stream[S_FFT], b->tap_bins.p, p);
        HIP_TRY(hipGetLastError());
    }
    b->late_attached.clear();
    return SDR_OK;
}


// A failure after the first launch leaves the pipeline half enqueued (some stages of this batch ran, the
// carried state of others did not advance): no later batch can be trusted, so the bank refuses further work.
int process_device_impl(sdr_bank *b, const void *iq_dev, int n_frames, size_t in_stride, sdr::InFormat fmt)
{
    if (b->failed)
        return fail(SDR_ERR_STATE, "an earlier process call failed half way; destroy the bank");
    if (b->graph_ready)
        return fail(SDR_ERR_STATE, "a graph is captured: process through sdr_graph_launch, or sdr_graph_release first");
    if (b->listen_pending)
        return fail(SDR_ERR_STATE, "the previous batch still waits for its listen half (sdr_process_listen)");
    const int rc = process_device_body(b, iq_dev, n_frames, in_stride, -1, -1, b->defer_listen ? PART_SPECTRA : PART_ALL, fmt);
    if (rc == SDR_ERR_HIP)
        b->failed = true;
    return rc;
}

namespace {

// One batch being enqueued: what it runs on (the bank, its buffer set, its plan), whether a capture is recording and which
// graph, and the batch's numbers - built by prepare_batch, read by the parts of process_device_body.  Its methods are the
// only place where a stage's waits, its kernel and its event are issued.
struct BatchIssue {
    sdr_bank *b;
    BatchSet *S;
    host::ResultSet *RS;  // (its block and events exist once bulk delivery is on)
    sdr::BatchPlan P;     // every choice of this batch (host/batch_plan.h) ...
    sdr::StageDeps deps;  // ... and who waits for whom
    // cap: the call is being recorded into graph `graph` (a stream's, or G_THRESHOLDS) as one batch of a replay.  Only the
    // kernels of that graph are issued, and NO event is recorded, waited for or queried - what orders the streams of a
    // replay are events around whole graphs (sdr_graph_launch).  cur: that batch's device-side cursor (else null).
    bool cap;
    int graph;
    int capture_k;
    sdr::BatchCursor *cur;
    int si, n_frames, max_slots, count0;
    int64_t first_frame;
    bool do_listen;
    sdr::CumGeom cg;

    // is kernel k part of the graph that is recording (always, outside a capture)?
    bool on(int k) const { return !cap || sdr::in_graph(P, k, graph); }
    hipStream_t stream(int k) const { return b->stream[P.stream[k]]; }
    // where stage k's last kernel goes: its stream and, outside a capture, the stage's event on the kernel's own dispatch
    sdr::LaunchAt at(int k) const { return sdr::LaunchAt(stream(k), cap ? nullptr : S->done[k]); }
    // stage k of this batch may start once stage `dep` of this batch is done (nothing to do on the same stream: under
    // SDR_NO_OVERLAP every stage's is the caller's)
    int wait(int k, int dep) const
    {
        if (!cap && stream(k) != stream(dep))
            HIP_TRY(hipStreamWaitEvent(stream(k), S->done[dep], 0));
        return SDR_OK;
    }
    // ... once every stage the plan orders it behind is
    int wait_deps(int k) const
    {
        for (int i = 0; i < deps.n; i++)
            if (deps.d[i].k == k)
                if (const int rc = wait(k, deps.d[i].dep))
                    return rc;
        return SDR_OK;
    }
    // stage k's event the ordinary way, where no kernel carries it
    int record(int k) const
    {
        if (!cap)
            HIP_TRY(hipEventRecord(S->done[k], stream(k)));
        return SDR_OK;
    }
    bool skipped(int k) const
    {
#if defined(SDR_DIAG)
        return (b->sw.diag_skip >> k & 1) != 0;
#else
        (void)k;
        return false;
#endif
    }
    // Stage k.  LAUNCH: `launch`, one launcher call, runs inside the stage's profile scope if the stage is on (and, in
    // -DSDR_DIAG builds, not skipped).  SCOPE_ONLY: the stage has a scope but no kernel of its own.  LEFT_OUT: neither.
    // carries: the launcher's last kernel takes the stage's event (else a plain launch: a kernel behind it, issued by the
    // caller, carries the event).  A stage that carries and launched nothing records its event the ordinary way: a stage
    // left out must still publish it - the set-reuse wait reads the last stage of each stream.
    enum Run { LAUNCH, SCOPE_ONLY, LEFT_OUT };
    template <class L>
    int stage(int k, Run how, bool carries, L &&launch) const
    {
        bool taken = false;
        if (how != LEFT_OUT) {
            ProfScope ps(b, k, stream(k));
            if (how == LAUNCH && on(k) && !skipped(k)) {
                const hipError_t e = launch(carries ? at(k) : sdr::LaunchAt(stream(k)));
                if (e != hipSuccess)
                    return fail(SDR_ERR_HIP, std::string("launch of stage ") + kKernelNames[k] + ": " + hipGetErrorString(e));
                taken = carries;
            }
        }
        return carries && !taken ? record(k) : SDR_OK;
    }
};

// capture_k >= 0: the batch is being recorded into a graph as its batch number capture_k (sdr_graph_capture).  Then it
// uses buffer set RING + capture_k, everything that differs from batch to batch comes from the device-side cursor of that
// number instead of the launch parameters and grids cover the most chunks a batch of this length can complete.
// Without PART_SPECTRA (the later listen half) set and first frame are the pending batch's (b->pend).
BatchIssue prepare_batch(sdr_bank *b, int n_frames, int capture_k, int capture_stage, bool do_spectra, bool do_listen, sdr::InFormat fmt)
{
    const sdr_config &c = b->cfg;
    BatchIssue is;
    is.b = b;
    is.cap = capture_k >= 0;
    is.graph = capture_stage;
    is.capture_k = capture_k;
    is.cur = is.cap ? b->cursors.p + capture_k : nullptr;
    is.si = is.cap ? RING + capture_k : do_spectra ? (int)(b->batch_index % RING) : b->pend.set;  // (capture: the sets sdr_graph_capture added)
    is.S = &b->set[is.si];
    is.RS = &b->results->set(is.si);
    is.n_frames = n_frames;
    is.first_frame = do_spectra ? b->total_frames : b->pend.first_frame;
    is.do_listen = do_listen;
    is.max_slots = 0;
    for (int i = 0; i < c.n_bands; i++)
        is.max_slots = std::max(is.max_slots, b->n_slots[i]);
    is.count0 = b->cum_count;
    is.P = sdr::plan_batch(b->sw, sdr::BatchGeometry{c.n_bands, c.block_size, c.max_batch_frames, b->max_chunks, b->fft_queue_alone}, n_frames, is.count0,
                           is.cap, is.max_slots, b->windowed, b->results_on ? b->row_columns : 0, b->results_on && b->reports_on, fmt, b->hop);
    is.deps = sdr::stage_deps(is.P, b->find_peaks && is.P.n_chunks > 0);
    is.cg = sdr::CumGeom{c.block_size, c.max_batch_frames, n_frames, is.count0, b->max_chunks};
    return is;
}

// The spectral half: FFT + PSD + tap, noise floor, thresholds.
int issue_spectra(const BatchIssue &is, const void *iq_dev, size_t in_stride)
{
    sdr_bank *b = is.b;
    const sdr_config &c = b->cfg;
    BatchSet &S = *is.S;
    const sdr::BatchPlan &P = is.P;
    const int B = c.n_bands, stride = c.max_batch_frames, n_frames = is.n_frames;
    // The FFT writes the set once every reader of it (batch i - RING) is done with it.  Not under capture: inside a graph
    // a set is used once per replay, and sdr_graph_launch waits for the earlier replay that used this phase's sets.
    if (!is.cap) {
        // With bulk delivery on, the set's previous batch must have been delivered (or be parked) before its block is
        // written again - and a delivered batch is a finished one: every reader of the set is done, the queries below
        // succeed and the FFT queue gets no barrier packets at all (each costs the command processor microseconds between
        // two FFT kernels, and the FFT queue is the one that bounds the step).
        if (b->results_on)
            if (const int rc = b->results->park(is.si))
                return rc;
        // With RING sets the previous user is four batches back and has almost always finished: ask the host first, a
        // barrier packet in the FFT queue costs the command processor tens of microseconds.
        // A caller that enqueues faster than the GPU works is soon more than RING batches ahead; then these events have
        // not happened yet at enqueue time and the FFT queue gets barrier packets: one per other stream (its last stage
        // stands for the stream: set_reuse_stages), not one per stage - with nothing else running that was 0.200 -> 0.177
        // ms per step for a 0.166 ms kernel.  (The host waiting instead - the call blocking until the set is free, the FFT
        // queue holding kernels only - was 0.161 ms with nothing else running, but 0.237 against 0.234 with the whole
        // pipeline, where the FFT launches are spaced by the CUs the tail holds, not by their queue.)
        int stands_for[N_STAGES];
        sdr::set_reuse_stages(P, stands_for);
        for (int k : stands_for)
            if (k >= 0 && hipEventQuery(S.done[k]) != hipSuccess)
                HIP_TRY(hipStreamWaitEvent(is.stream(sdr::K_FFT), S.done[k], 0));
    }
    if (is.cap && is.on(sdr::K_FFT) && is.capture_k % RING == 0)  // the replay's cursors, in front of its first FFT
        HIP_TRY(launch_set_cursors(is.cur, CursorPack{}, is.stream(sdr::K_FFT)));
    const sdr::FftLaunch fl{b->logn, P.fft, iq_dev, is.cur, b->tw.p, S.psd.p, n_frames, B, in_stride, b->hop, stride,
                            sdr::FftTap{b->tap_bins.p, S.tap.p, is.max_slots, c.max_listeners, S.tapw.p, S.tap_used.p},
                            S.fft_ctr.p, S.fft_scratch.p, b->windowed ? b->window.p : nullptr};
    // (n_frames > 0, process_device_body: launch_fft and launch_psd_scan launch nothing for an empty batch and would leave
    // the event they are given unrecorded)
    int rc = is.stage(sdr::K_FFT, BatchIssue::LAUNCH, true, [&](sdr::LaunchAt at) { return sdr::launch_fft(fl, at); });
    if (rc)
        return rc;

    // noise floor (stateless per batch), then the rolling means -> thresholds, in batch order.  Two ways:
    //   scan    k_noise_scan.hip: ONE pass over the psd for FindNoiseFloor's sums and - where it pays - the bounds of the
    //           cumulations the batch completes; the reference's values where they are consumed (noise_cert.h), the
    //           literal loops for the few frames that cannot be certified;
    //   chains  k_noise.hip: the ordered float64 chains of rounds 1-4 (and k_cum_bound on the peaks stream).
    const sdr::NoiseGeom ng = b->noise_geom();
    if ((rc = is.wait_deps(sdr::K_WINDOW_MEANS)))
        return rc;
    rc = is.stage(sdr::K_WINDOW_MEANS, BatchIssue::LAUNCH, true, [&](sdr::LaunchAt at) {
        if (P.noise_scan)
            return sdr::launch_psd_scan(S.psd.p, S.recs.p, S.cum_out.p, S.cum_part.p, is.cur, ng, is.cg, P.n_slots, B, P.bound_done, P.scan_parts,
                                        P.force_exact, at);
        return sdr::launch_window_means(S.psd.p, S.win_mean.p, ng, n_frames, B, stride, P.wm_wpb, at);
    });
    if (rc || (rc = is.wait_deps(sdr::K_NOISE_STATS)))
        return rc;
    // (the scan kernel has finished the records itself: then this stage launches nothing and its event is recorded)
    rc = is.stage(sdr::K_NOISE_STATS, P.noise_scan ? BatchIssue::SCOPE_ONLY : BatchIssue::LAUNCH, true, [&](sdr::LaunchAt at) {
        return sdr::launch_noise_stats(S.psd.p, S.win_mean.p, S.recs.p, ng, n_frames, B, stride, P.var_mfma, at);
    });
    if (rc || (rc = is.wait_deps(sdr::K_THRESHOLDS)))
        return rc;
    return is.stage(sdr::K_THRESHOLDS, BatchIssue::LAUNCH, true,
                    [&](sdr::LaunchAt at) { return sdr::launch_thresholds(S.recs.p, b->band_state.p, n_frames, B, stride, at); });
}

// The listen half: per-signal envelope + decoder, and their delivery.
int issue_listen(const BatchIssue &is)
{
    sdr_bank *b = is.b;
    const sdr_config &c = b->cfg;
    BatchSet &S = *is.S;
    const int B = c.n_bands, n_frames = is.n_frames, max_slots = is.max_slots;
    const BatchIssue::Run run = max_slots > 0 ? BatchIssue::LAUNCH : BatchIssue::LEFT_OUT;
    sdr::ListenGeom lg;
    lg.n = c.block_size;
    lg.stride = c.max_batch_frames;
    lg.max_listeners = c.max_listeners;
    lg.text_cap = b->text_cap;
    lg.edge_cap = b->edge_cap;
    lg.bit_words = b->bit_words;
    lg.trace = c.trace;
    lg.frame_base = (uint32_t)is.first_frame;
    int rc = is.wait_deps(sdr::K_LISTEN_GATHER);
    if (rc)
        return rc;
    // Slots of listeners bound by sdr_attach_at: the gather reads a slot's active, bin, start_frame and tapped_from, and
    // k_put_slots writes them word by word on the listen stream (flush_late_attached, this call's or an earlier one's).
    // The waits above say nothing about that stream, and the listen stream of a small plan runs a batch or more behind
    // the peaks stream, so a gather elsewhere waits for the last put until the host has seen it complete.  The other slot
    // writers on the listen stream need no such wait: k_set_debounce writes deb.threshold, k_listener_stop dec /
    // text_count / text_dropped, and k_listen_decode of the batch before moves start_frame and tapped_from of a listener
    // that has started from a frame at or before that batch's first to this batch's first - old or new, the gather
    // skips no frame and reads every one from the tap; sdr_attach and sdr_detach write slots only after sync_bank has
    // drained every stream.
    if (!is.cap && b->slots_put) {
        if (hipEventQuery(b->slots_put_ev) == hipSuccess)
            b->slots_put = false;
        else if (is.P.stream[sdr::K_LISTEN_GATHER] != S_LISTEN)
            HIP_TRY(hipStreamWaitEvent(is.stream(sdr::K_LISTEN_GATHER), b->slots_put_ev, 0));
    }
    rc = is.stage(sdr::K_LISTEN_GATHER, run, true, [&](sdr::LaunchAt at) {
        return sdr::launch_listen_gather(S.tap.p, S.psd.p, S.recs.p, b->slots.p, b->db_tab.p, S.raw_bits.p, S.tr_values.p, S.tr_raw.p, is.cur, lg, n_frames,
                                         max_slots, B, at);
    });
    if (rc || (rc = is.wait_deps(sdr::K_LISTEN_DECODE)))
        return rc;
    if (c.trace && max_slots > 0 && is.on(sdr::K_LISTEN_DECODE))  // the decoders' state before this batch: the decoder scope replays from it
        HIP_TRY(hipMemcpyAsync(S.slots_before.p, b->slots.p, sizeof(sdr::ListenerSlot) * (size_t)B * (size_t)c.max_listeners, hipMemcpyDeviceToDevice,
                               is.stream(sdr::K_LISTEN_DECODE)));
    // listener reports: where every listener starts and is tapped from in this batch, before the decoder moves the marks
    const bool reports = is.P.reports && run == BatchIssue::LAUNCH && is.on(sdr::K_LISTEN_DECODE) && !is.skipped(sdr::K_LISTEN_DECODE);
    if (reports) {
        ProfScope ps(b, sdr::K_REPORT_MARKS, b->stream[is.P.reports_stream]);
        HIP_TRY(sdr::launch_report_marks(b->slots.p, is.cur, lg, n_frames, B, S.report_marks.p, b->stream[is.P.reports_stream]));
    }
    // (with bulk delivery the stage's event rides on the pack kernel below, not on the decoder)
    rc = is.stage(sdr::K_LISTEN_DECODE, run, !b->results_on, [&](sdr::LaunchAt at) {
        return sdr::launch_listen_decode(b->slots.p, b->morse.p, S.raw_bits.p, S.bits.p, b->text.p, b->text_frames.p, S.edges.p, S.edge_counts.p, S.tr_deb.p,
                                         b->drops.p, is.cur, lg, n_frames, B, b->edge_pos.p, c.max_batch_frames, at);
    });
    if (rc)
        return rc;
    // ... and the reports themselves, straight into the set's report block: behind the decoder, in front of the pack kernel
    // and so in front of the event sdr_poll looks at
    if (reports) {
        ProfScope ps(b, sdr::K_LISTEN_REPORT, b->stream[is.P.reports_stream]);
        HIP_TRY(sdr::launch_listen_report(S.tap.p, S.psd.p, S.recs.p, b->slots.p, b->db_tab.p, S.bits.p, S.report_marks.p, lg, n_frames, max_slots, B,
                                          is.RS->reports, b->stream[is.P.reports_stream]));
    }
    if (b->results_on && is.on(sdr::K_LISTEN_DECODE)) {
        // delivery of this batch's edges and runes, behind the decoder on its stream; the decoder's event is
        // recorded behind it so that the set is not reused before the copy to the host has happened
        HIP_TRY(sdr::launch_pack_listen(b->slots.p, S.edges.p, S.edge_counts.p, b->text.p, b->text_frames.p, b->drops.p, b->res_layout, max_slots, B,
                                        is.RS->block, is.at(sdr::K_LISTEN_DECODE)));
        if (!is.cap)  // (a replay records it behind the listen graph)
            HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(is.RS->ev_listen), is.stream(sdr::K_LISTEN_DECODE)));
    }
    return SDR_OK;
}

// dB projection + cumulation, peak scan (rx/receiver.go:404-409,459-460), the waterfall rows and their delivery.
int issue_cumulation(const BatchIssue &is)
{
    sdr_bank *b = is.b;
    const sdr_config &c = b->cfg;
    BatchSet &S = *is.S;
    const sdr::BatchPlan &P = is.P;
    const int B = c.n_bands, n_frames = is.n_frames, n_chunks = P.n_chunks;
    // (the scan wrote the bounds of the completed cumulations on the noise stream: the carry is added to slot 0's here)
    int rc = is.wait_deps(sdr::K_CUMULATE);
    if (rc)
        return rc;
    rc = is.stage(sdr::K_CUMULATE, BatchIssue::LAUNCH, true, [&](sdr::LaunchAt at) {
        return sdr::launch_cumulate(S.psd.p, b->db_tab.p, b->carry[0].p, b->carry[1].p, b->carry_cur, S.cum_out.p, S.cum_part.p, is.cur, is.cg, P.n_slots, B,
                                    P.bound, P.bound_done, P.scan_parts, at);
    });
    if (rc || (rc = is.wait_deps(sdr::K_FIND_PEAKS)))
        return rc;
    // (n_chunks > 0: launch_find_peaks launches nothing without a completed cumulation and would leave its event unrecorded;
    // with bulk delivery the stage's event rides on the pack kernel below)
    const bool peak_scan = b->find_peaks && n_chunks > 0;
    rc = is.stage(sdr::K_FIND_PEAKS, peak_scan ? BatchIssue::LAUNCH : BatchIssue::LEFT_OUT, !b->results_on, [&](sdr::LaunchAt at) {
        sdr::PeakGeom pg{c.block_size, c.max_batch_frames, is.count0, b->max_chunks, c.max_peaks};
        // (reads the carry buffer this batch's cumulation started from: the next batch's k_cumulate, which writes that
        // buffer, follows on the same stream)
        // the wide tap this batch's FFT left, if it was the kernel that leaves one (k_cum_refine reads the signals' columns there)
        sdr::FftTap wide_tap{nullptr, nullptr, is.max_slots, c.max_listeners};
        if (P.fft.wide_tap) {
            wide_tap.wide = S.tapw.p;
            wide_tap.used = S.tap_used.p;
        }
        return sdr::launch_find_peaks(S.cum_out.p, S.psd.p, b->db_tab.p, b->carry[0].p, b->carry[1].p, b->carry_cur, S.recs.p, S.dev_peaks.p,
                                      S.peak_counts.p, is.cur, pg, n_frames, n_chunks, B, P.refine, wide_tap, at);
    });
    if (rc)
        return rc;
    if (!is.on(sdr::K_FIND_PEAKS))
        return SDR_OK;
    // the waterfall rows of the completed cumulations, straight into the set's row block: behind the cumulate step on the
    // find-peaks stage's stream, in front of the event sdr_poll looks at (recorded behind the pack kernel below)
    if (P.rows) {
        ProfScope ps(b, sdr::K_CUM_ROWS, b->stream[P.rows_stream]);
        HIP_TRY(sdr::launch_cum_rows(S.psd.p, b->db_tab.p, b->carry[0].p, b->carry[1].p, b->carry_cur, is.cur, is.cg, b->row_columns, n_chunks, B, is.RS->rows,
                                     b->stream[P.rows_stream]));
    }
    if (!b->results_on)
        return SDR_OK;
    // delivery of this batch's peaks, with the stage's event.  launch_pack_peaks launches nothing for a batch that completes
    // no cumulation: then the event is recorded the ordinary way, at the end
    if (n_chunks > 0)
        HIP_TRY(sdr::launch_pack_peaks(S.dev_peaks.p, S.peak_counts.p, is.cur, b->res_layout, b->find_peaks, n_frames, n_chunks, B, is.RS->block,
                                       is.at(sdr::K_FIND_PEAKS)));
    if (!is.cap) {
        HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(is.RS->ev_peaks), is.stream(sdr::K_FIND_PEAKS)));
        host::BatchMeta m;
        m.batch = b->batch_index;
        m.first_frame = b->total_frames;
        m.frames = n_frames;
        m.chunks = n_chunks;
        m.count0 = is.count0;
        m.slots = is.do_listen ? is.max_slots : 0;  // (sdr_poll_peaks delivers the spectral half; the listen half fills this in)
        m.row_columns = P.rows ? b->row_columns : 0;
        m.rows = P.rows ? n_chunks * B : 0;
        m.reports = P.reports && is.do_listen ? 1 : 0;  // (a deferred listen half says so itself: Delivery::complete)
        m.report_bands = B;
        m.report_stride = c.max_listeners;
        {
            std::lock_guard<std::mutex> guard(b->center_mu);
            m.center = b->center_frequency;
        }
        b->results->publish(is.si, std::move(m), is.do_listen);
    }
    return n_chunks > 0 ? SDR_OK : is.record(sdr::K_FIND_PEAKS);
}

// Every launch of the batch is enqueued: commit the host's view of the carried state in one go.
// The carry buffer flips only when this batch wrote a new partial cumulation; if the batch ended
// exactly on a chunk boundary the next batch starts from zero (count0 == 0 ignores the carry)
void commit_batch(const BatchIssue &is)
{
    sdr_bank *b = is.b;
    b->last_carry_in = b->carry_cur;
    if (is.P.new_count != 0)
        b->carry_cur ^= 1;
    b->cum_count = is.P.new_count;
    b->last_set = is.si;
    b->last_frames = is.n_frames;
    b->last_chunks = is.P.n_chunks;
    b->last_count0 = is.count0;
    b->last_edge_width = b->edge_width;
    if (!is.do_listen) {
        b->pend.set = is.si;
        b->pend.frames = is.n_frames;
        b->pend.first_frame = b->total_frames;
        b->pend.batch = b->batch_index;
        b->listen_pending = true;
    }
    b->total_frames += is.n_frames;
    b->batch_index++;
    if (!b->results_on)
        b->results->note_enqueued(b->batch_index);
}

}  // namespace

// One batch, or the parts of it that `parts` names.  capture_k >= 0 / capture_stage: the call is being recorded into the
// graph of stream capture_stage (or G_THRESHOLDS) as batch capture_k of a replay (sdr_graph_capture walks the batches once
// per graph; see BatchIssue::cap): nothing is asked of the host (no event queries, no profiling, no parking, no late-attach
// flush) and no host state changes.
// parts: PART_SPECTRA leaves the batch's listeners for a later PART_LISTEN call (sdr_defer_listen / sdr_process_listen:
// the host binds listeners to peaks of this very batch in between, rx/receiver.go:409-426); the later call takes the
// batch's set, length and first frame from b->pend.
int process_device_body(sdr_bank *b, const void *iq_dev, int n_frames, size_t in_stride, int capture_k, int capture_stage, int parts,
                        sdr::InFormat fmt)
{
    const bool cap = capture_k >= 0;
    const bool do_spectra = (parts & PART_SPECTRA) != 0, do_listen = (parts & PART_LISTEN) != 0;
    if (!do_spectra)
        n_frames = b->pend.frames;
    if (n_frames <= 0)  // (no launcher is ever called for an empty batch)
        return SDR_OK;
    if (n_frames > b->cfg.max_batch_frames)
        return fail(SDR_ERR_BAD_ARG, "n_frames exceeds max_batch_frames");
    HIP_TRY(hipSetDevice(b->device));
    if (!cap)
        if (const int rc = flush_late_attached(b))
            return rc;
    const BatchIssue is = prepare_batch(b, n_frames, capture_k, capture_stage, do_spectra, do_listen, fmt);
    int rc;
    if (do_spectra && (rc = issue_spectra(is, iq_dev, in_stride)))
        return rc;
    if (do_listen && (rc = issue_listen(is)))
        return rc;
    if (!do_spectra) {
        // the batch is complete: sdr_poll may have it
        b->results->complete(is.si, is.max_slots, b->pend.batch, is.P.reports ? 1 : 0);
        b->listen_pending = false;
        return SDR_OK;
    }
    if ((rc = issue_cumulation(is)))
        return rc;
    if (!cap)
        commit_batch(is);
    return SDR_OK;
}

}  // namespace sdrcapi

extern "C" {
#pragma GCC visibility push(default)

namespace {
static int check_device_input(sdr_bank *b, const void *iq_dev)
{
    if (!b || !iq_dev)
        return fail(SDR_ERR_BAD_ARG, "null argument");
    if (reinterpret_cast<uintptr_t>(iq_dev) & 15)
        return fail(SDR_ERR_BAD_ARG, "iq_dev must be 16-byte aligned (frames are copied to LDS 16 bytes per lane)");
    return SDR_OK;
}
static int process_device_dense(sdr_bank *b, const void *iq_dev, int n_frames, sdr::InFormat fmt)
{
    const int rc = check_device_input(b, iq_dev);
    if (rc)
        return rc;
    if (b->hop != b->cfg.block_size)
        return fail(SDR_ERR_STATE, "the bank's frames overlap (hop < block_size): [band][frame] input has no meaning, use sdr_process_device_stream");
    return process_device_impl(b, iq_dev, n_frames, (size_t)std::max(n_frames, 0) * (size_t)b->cfg.block_size, fmt);
}
static int process_device_stream(sdr_bank *b, const void *iq_dev, int n_frames, size_t band_stride_samples, sdr::InFormat fmt)
{
    const int rc = check_device_input(b, iq_dev);
    if (rc)
        return rc;
    if (band_stride_samples % (sdr::is_iq8(fmt) ? 8 : 4) != 0)
        return fail(SDR_ERR_BAD_ARG, sdr::is_iq8(fmt) ? "band_stride_samples must be a multiple of 8 samples (every band's stream 16-byte aligned)"
                                                      : "band_stride_samples must be a multiple of 4 samples (every band's stream 16-byte aligned)");
    if (band_stride_samples < sdr::span_samples(n_frames, b->hop, b->cfg.block_size) || band_stride_samples > 0xffffffffu)
        return fail(SDR_ERR_BAD_ARG, "band_stride_samples is smaller than (n_frames - 1) * hop + block_size (or beyond 2^32 - 1)");
    return process_device_impl(b, iq_dev, n_frames, band_stride_samples, fmt);
}
}  // namespace

int sdr_process_device(sdr_bank *b, const float *iq_dev, int n_frames) { return process_device_dense(b, iq_dev, n_frames, sdr::InFormat::F32); }

int sdr_process_device_sc16(sdr_bank *b, const int16_t *iq_dev, int n_frames)
{
    return process_device_dense(b, iq_dev, n_frames, sdr::InFormat::SC16);
}

int sdr_process_device_stream(sdr_bank *b, const float *iq_dev, int n_frames, size_t band_stride_samples)
{
    return process_device_stream(b, iq_dev, n_frames, band_stride_samples, sdr::InFormat::F32);
}

int sdr_process_device_stream_sc16(sdr_bank *b, const int16_t *iq_dev, int n_frames, size_t band_stride_samples)
{
    return process_device_stream(b, iq_dev, n_frames, band_stride_samples, sdr::InFormat::SC16);
}

int sdr_process_device_iq8(sdr_bank *b, const void *iq_dev, int n_frames, int format)
{
    sdr::InFormat fmt;
    if (const int rc = iq8_format(format, &fmt))
        return rc;
    return process_device_dense(b, iq_dev, n_frames, fmt);
}

int sdr_process_device_stream_iq8(sdr_bank *b, const void *iq_dev, int n_frames, size_t band_stride_samples, int format)
{
    sdr::InFormat fmt;
    if (const int rc = iq8_format(format, &fmt))
        return rc;
    return process_device_stream(b, iq_dev, n_frames, band_stride_samples, fmt);
}

int sdr_hop(sdr_bank *b) { return b ? b->hop : -1; }


// ---- deferred listen half: strain-mode discovery without a host round trip per cumulation -----------------------
// rx/receiver.go:409-426 binds one listener per completed cumulation, to a peak of that cumulation, and the listener
// hears the very next frame.  Frame by frame that is a decision on the host every 100 frames.  Here the spectral half
// of a long batch runs first (FFT .. FindPeaks of EVERY cumulation in it), the host reads those peaks (sdr_poll_peaks),
// makes the same decisions in the same order and binds each listener with the frame it starts at (sdr_attach_at); then
// the listen half runs over the retained spectra (sdr_process_listen).  Listeners are independent of each other, so a
// listener that starts in the middle of the batch produces exactly what it would have produced attached there live.
int sdr_defer_listen(sdr_bank *b, int on)
{
    if (!b)
        return fail(SDR_ERR_BAD_ARG, "null bank");
    if (on && !b->results_on)
        return fail(SDR_ERR_STATE, "deferred listening needs bulk delivery (sdr_enable_results)");
    if (b->listen_pending)
        return fail(SDR_ERR_STATE, "a batch waits for its listen half (sdr_process_listen)");
    b->defer_listen = on != 0;
    return SDR_OK;
}

int sdr_listen_pending(sdr_bank *b) { return b && b->listen_pending ? 1 : 0; }

int sdr_process_listen(sdr_bank *b)
{
    if (!b)
        return fail(SDR_ERR_BAD_ARG, "null bank");
    if (b->failed)
        return fail(SDR_ERR_STATE, "an earlier process call failed half way; destroy the bank");
    if (!b->listen_pending)
        return fail(SDR_ERR_STATE, "no batch waits for its listen half");
    const int rc = process_device_body(b, nullptr, b->pend.frames, 0, -1, -1, PART_LISTEN);  // (no FFT: no input)
    if (rc == SDR_ERR_HIP)
        b->failed = true;
    return rc;
}


#pragma GCC visibility pop
}  // extern "C"
