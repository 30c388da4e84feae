// capi_group.hip — sdr_group (include/sdrainer_hip.h): one bank per member device, driven as one bank of n_bands bands
// from one host process - the single-process counterpart of sharding.ShardedBank, reachable from a C or Go host.
// Built on the public bank ABI only: every member is an ordinary sdr_bank, and there is no device work of the group's
// own.  Routing, the frame count of a staged call and the merge / park logic of delivery are host/group.h (plain C++,
// exercised without a GPU by tests/host/test_group.cpp); this file is the C ABI in front of it: the checks that keep the
// members in step, the fan-out to the members, and the caller's current device.
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "../../include/sdrainer_hip.h"
#include "host/group.h"

namespace sdr {
int set_error(int code, const char *msg);  // capi_bank.hip: the calling thread's sdr_last_error()
}  // namespace sdr

namespace {

struct BankSource final : host::GroupSource {
    std::vector<sdr_bank *> *banks;
    explicit BankSource(std::vector<sdr_bank *> *b) : banks(b) {}
    int poll(int m, sdr_results *r, bool wait) override { return sdr_poll((*banks)[(size_t)m], r, wait ? 1 : 0); }
    int poll_peaks(int m, sdr_results *r, bool wait) override { return sdr_poll_peaks((*banks)[(size_t)m], r, wait ? 1 : 0); }
    int poll_rows(int m, float *rows, int rows_cap, int *n_rows, int64_t *batch_index, bool wait) override
    {
        return sdr_poll_rows((*banks)[(size_t)m], rows, rows_cap, n_rows, batch_index, wait ? 1 : 0);
    }
    int poll_reports(int m, sdr_listener_report *out, int cap, int *n_out, int64_t *batch_index, bool wait) override
    {
        return sdr_poll_reports((*banks)[(size_t)m], out, cap, n_out, batch_index, wait ? 1 : 0);
    }
    int report(int code, const char *msg) override { return sdr::set_error(code, msg); }
};

// Every group call leaves the caller's current HIP device as it found it (the members' calls select theirs).
struct KeepDevice {
    int dev = -1;
    KeepDevice()
    {
        if (hipGetDevice(&dev) != hipSuccess)
            dev = -1;
    }
    ~KeepDevice()
    {
        if (dev >= 0)
            (void)hipSetDevice(dev);
    }
};

// A 16-byte aligned address for a zero-frame sdr_process_device: the bank checks its state (failed, graph captured,
// listen half pending) and returns before it reads or launches anything.
alignas(16) float g_probe[4];

}  // namespace

struct sdr_group {
    sdr_config cfg{};
    host::GroupRouting rt;
    std::vector<sdr_bank *> banks;
    std::unique_ptr<BankSource> src;
    std::unique_ptr<host::GroupDelivery> delivery;
    bool failed = false;  // producer-owned: a member failed after another had run, the members are out of step
};

namespace {

int fail(int code, const char *msg) { return sdr::set_error(code, msg); }

int route(sdr_group *g, int band, sdr_bank **bank, int *local)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    if (band < 0 || band >= g->rt.n_bands)
        return fail(SDR_ERR_BAD_ARG, "band out of range");
    *bank = g->banks[(size_t)g->rt.member_of(band)];
    *local = g->rt.local_of(band);
    return SDR_OK;
}

// Before any member is launched: the group has not failed and every member may process a new batch.
int check_members(sdr_group *g)
{
    if (g->failed)
        return fail(SDR_ERR_STATE, "an earlier group call left the members out of step; destroy the group");
    for (sdr_bank *b : g->banks) {
        const int rc = sdr_process_device(b, g_probe, 0);
        if (rc)
            return rc;  // (SDR_ERR_STATE: graph captured, listen half pending, or the member failed on its own)
    }
    return SDR_OK;
}

// A member call failed: once another member has run this batch, or on a HIP failure, the members are out of step.
int member_failed(sdr_group *g, int rc, int member)
{
    if (rc == SDR_ERR_HIP || member > 0)
        g->failed = true;
    return rc;
}

// One band's push: the band's member and local band, the caller's device kept, then the member's call.
template <class Push>
int push_to_member(sdr_group *g, int band, Push &&push)
{
    sdr_bank *b = nullptr;
    int local = 0;
    const int rc = route(g, band, &b, &local);
    if (rc)
        return rc;
    KeepDevice keep;
    return push(b, local);
}

// iq_dev: one pointer per member, frames of one kind; process: the member call that takes them
template <class Process>
int group_process_device(sdr_group *g, const void *const *iq_dev, int n_frames, Process &&process)
{
    if (!g || !iq_dev)
        return fail(SDR_ERR_BAD_ARG, "null argument");
    for (int m = 0; m < g->rt.n_members; m++) {
        if (!iq_dev[m])
            return fail(SDR_ERR_BAD_ARG, "null iq_dev of a member");
        if (reinterpret_cast<uintptr_t>(iq_dev[m]) & 15)
            return fail(SDR_ERR_BAD_ARG, "iq_dev must be 16-byte aligned (frames are copied to LDS 16 bytes per lane)");
    }
    if (n_frames > g->cfg.max_batch_frames)
        return fail(SDR_ERR_BAD_ARG, "n_frames exceeds max_batch_frames");
    KeepDevice keep;
    int rc = check_members(g);
    if (rc)
        return rc;
    if (n_frames <= 0)
        return SDR_OK;
    // (sdr_process_device only enqueues: every member is launched before anything is waited for)
    for (int m = 0; m < g->rt.n_members; m++) {
        rc = process(g->banks[(size_t)m], iq_dev[m], n_frames);
        if (rc)
            return member_failed(g, rc, m);
    }
    return SDR_OK;
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int sdr_group_create(const sdr_config *cfg, const int32_t *device_ids, int n_members, sdr_group **out)
{
    if (!cfg || !device_ids || !out)
        return fail(SDR_ERR_BAD_ARG, "null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(sdr_config))
        return fail(SDR_ERR_BAD_ARG, "sdr_config.struct_size mismatch (ABI)");
    if (cfg->hop != 0 && cfg->hop != cfg->block_size)  // (the group's device call takes [band][frame] batches per member)
        return fail(SDR_ERR_BAD_ARG, "a group is not offered with hop < block_size (overlapped frames)");
    host::GroupRouting rt{cfg->n_bands, n_members};
    if (!rt.valid())
        return fail(SDR_ERR_BAD_ARG, "a group needs at least one member and at least one band per member");
    KeepDevice keep;
    std::unique_ptr<sdr_group> g(new sdr_group);
    g->cfg = *cfg;
    g->rt = rt;
    for (int m = 0; m < n_members; m++) {
        sdr_config mc = *cfg;
        mc.n_bands = rt.bands_of(m);
        mc.device_id = device_ids[m];
        sdr_bank *b = nullptr;
        const int rc = sdr_create(&mc, &b);
        if (rc) {
            for (sdr_bank *made : g->banks)
                sdr_destroy(made);
            return rc;
        }
        g->banks.push_back(b);
    }
    g->src.reset(new BankSource(&g->banks));
    g->delivery.reset(new host::GroupDelivery(g->src.get(), rt));
    *out = g.release();
    return SDR_OK;
}

int sdr_group_destroy(sdr_group *g)
{
    if (!g)
        return SDR_OK;
    KeepDevice keep;
    int rc = SDR_OK;
    for (sdr_bank *b : g->banks) {
        const int r = sdr_destroy(b);
        rc = rc ? rc : r;
    }
    delete g;
    return rc;
}

int sdr_group_member(sdr_group *g, int band, sdr_bank **bank, int *local_band)
{
    if (!bank || !local_band)
        return fail(SDR_ERR_BAD_ARG, "null argument");
    return route(g, band, bank, local_band);
}

int sdr_group_push_iq(sdr_group *g, int band, int sample_rate, const float *iq, size_t n_floats)
{
    return push_to_member(g, band, [&](sdr_bank *b, int local) { return sdr_push_iq(b, local, sample_rate, iq, n_floats); });
}

int sdr_group_push_iq_sc16(sdr_group *g, int band, int sample_rate, const int16_t *iq, size_t n_values)
{
    return push_to_member(g, band, [&](sdr_bank *b, int local) { return sdr_push_iq_sc16(b, local, sample_rate, iq, n_values); });
}

int sdr_group_push_iq8(sdr_group *g, int band, int sample_rate, const void *iq, size_t n_values, int format)
{
    return push_to_member(g, band, [&](sdr_bank *b, int local) { return sdr_push_iq8(b, local, sample_rate, iq, n_values, format); });
}

int sdr_group_push_kiwi_snd(sdr_group *g, int band, int sample_rate, const uint8_t *payload, size_t n_bytes)
{
    return push_to_member(g, band, [&](sdr_bank *b, int local) { return sdr_push_kiwi_snd(b, local, sample_rate, payload, n_bytes); });
}

int sdr_group_process_staged(sdr_group *g, int *n_frames_out)
{
    return sdr_group_process_staged_limit(g, g ? g->cfg.max_batch_frames : 0, n_frames_out);
}

int sdr_group_process_staged_limit(sdr_group *g, int max_frames, int *n_frames_out)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    if (n_frames_out)
        *n_frames_out = 0;
    KeepDevice keep;
    int rc = check_members(g);
    if (rc)
        return rc;
    std::vector<int> staged((size_t)g->rt.n_bands);
    for (int band = 0; band < g->rt.n_bands; band++)
        staged[(size_t)band] = sdr_staged_frames(g->banks[(size_t)g->rt.member_of(band)], g->rt.local_of(band));
    const int n = host::group_frames(staged, max_frames, g->cfg.max_batch_frames);
    if (n_frames_out)
        *n_frames_out = n;
    if (n == 0)
        return SDR_OK;
    for (int m = 0; m < g->rt.n_members; m++) {
        int done = 0;
        rc = sdr_process_staged_limit(g->banks[(size_t)m], n, &done);
        if (rc)
            return member_failed(g, rc, m);
        if (done != n) {
            g->failed = true;
            return fail(SDR_ERR_STATE, "a member consumed another frame count than the group (out of step)");
        }
    }
    return SDR_OK;
}

int sdr_group_process_device(sdr_group *g, const float *const *iq_dev, int n_frames)
{
    return group_process_device(g, reinterpret_cast<const void *const *>(iq_dev), n_frames,
                                [](sdr_bank *b, const void *iq, int n) { return sdr_process_device(b, static_cast<const float *>(iq), n); });
}

int sdr_group_process_device_sc16(sdr_group *g, const int16_t *const *iq_dev, int n_frames)
{
    return group_process_device(g, reinterpret_cast<const void *const *>(iq_dev), n_frames,
                                [](sdr_bank *b, const void *iq, int n) { return sdr_process_device_sc16(b, static_cast<const int16_t *>(iq), n); });
}

int sdr_group_process_device_iq8(sdr_group *g, const void *const *iq_dev, int n_frames, int format)
{
    if (format != SDR_IQ8_CS8 && format != SDR_IQ8_CU8)
        return fail(SDR_ERR_BAD_ARG, "format must be SDR_IQ8_CS8 or SDR_IQ8_CU8");
    return group_process_device(g, iq_dev, n_frames, [format](sdr_bank *b, const void *iq, int n) { return sdr_process_device_iq8(b, iq, n, format); });
}

int sdr_group_sync(sdr_group *g)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    KeepDevice keep;
    for (sdr_bank *b : g->banks) {
        const int rc = sdr_sync(b);
        if (rc)
            return rc;
    }
    return SDR_OK;
}

// Collective setters.  A bank applies a setter at its next process call; the group's next process call runs every
// member, so every band changes at the same frame.  The members share one geometry: what the first accepts, all accept.
int sdr_group_set_peak_threshold(sdr_group *g, int band, float threshold)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    if (band < -1 || band >= g->rt.n_bands)
        return fail(SDR_ERR_BAD_ARG, "band out of range (-1: every band)");
    KeepDevice keep;
    for (int b = band < 0 ? 0 : band; b < (band < 0 ? g->rt.n_bands : band + 1); b++) {
        const int rc = sdr_set_peak_threshold(g->banks[(size_t)g->rt.member_of(b)], g->rt.local_of(b), threshold);
        if (rc)
            return rc;
    }
    return SDR_OK;
}

int sdr_group_set_signal_debounce(sdr_group *g, int band, int debounce)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    if (band < -1 || band >= g->rt.n_bands)
        return fail(SDR_ERR_BAD_ARG, "band out of range (-1: every band)");
    for (sdr_bank *b : g->banks)  // (refused before any member changes, as sdr_group_set_window is)
        if (sdr_listen_pending(b))
            return fail(SDR_ERR_STATE, "a batch waits for its listen half (sdr_group_process_listen)");
    KeepDevice keep;
    for (int b = band < 0 ? 0 : band; b < (band < 0 ? g->rt.n_bands : band + 1); b++) {
        const int rc = sdr_set_signal_debounce(g->banks[(size_t)g->rt.member_of(b)], g->rt.local_of(b), debounce);
        if (rc)
            return rc;
    }
    return SDR_OK;
}

int sdr_group_set_edge_width(sdr_group *g, int edge_width)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    KeepDevice keep;
    for (sdr_bank *b : g->banks) {
        const int rc = sdr_set_edge_width(b, edge_width);
        if (rc)
            return rc;
    }
    return SDR_OK;
}

int sdr_group_set_window(sdr_group *g, const float *window, int n)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    // What a member could refuse is checked for all of them before any table changes: the arguments are judged against
    // the one geometry they share by the first member, a listen half is pending on every member or on none, and the
    // group offers no graph capture.
    for (sdr_bank *b : g->banks)
        if (sdr_listen_pending(b))
            return fail(SDR_ERR_STATE, "a batch waits for its listen half (sdr_group_process_listen)");
    KeepDevice keep;
    for (sdr_bank *b : g->banks) {
        const int rc = sdr_set_window(b, window, n);
        if (rc)
            return rc;
    }
    return SDR_OK;
}

int sdr_group_set_find_peaks(sdr_group *g, int on)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    KeepDevice keep;
    for (sdr_bank *b : g->banks) {
        const int rc = sdr_set_find_peaks(b, on);
        if (rc)
            return rc;
    }
    return SDR_OK;
}

// The members cannot come to disagree: where one refuses, those set before it (fresh banks, or they had refused) get
// the frame they had back.
int sdr_group_set_first_frame(sdr_group *g, int64_t frame)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    std::vector<int64_t> before;
    for (sdr_bank *b : g->banks) {
        before.push_back(sdr_total_frames(b));
        const int rc = sdr_set_first_frame(b, frame);
        if (rc) {
            for (size_t m = 0; m + 1 < before.size(); m++)
                (void)sdr_set_first_frame(g->banks[m], before[m]);
            return rc;  // (the member's message stands: a successful call leaves it alone)
        }
    }
    return SDR_OK;
}

int sdr_group_enable_results(sdr_group *g, int on)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    KeepDevice keep;
    for (sdr_bank *b : g->banks) {
        const int rc = sdr_enable_results(b, on);
        if (rc)
            return rc;
    }
    g->delivery->reset(on != 0);  // (undelivered batches are discarded with the mode, as every member discards its own)
    if (!on)
        g->delivery->set_rows(0);  // (the members switched their rows off with the results)
    if (!on)
        g->delivery->set_reports(false);  // (... and their reports)
    return SDR_OK;
}

int sdr_group_enable_rows(sdr_group *g, int columns)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    // what a member could refuse is checked for all of them first: they share one geometry and one delivery mode, and a
    // listen half is pending on every member or on none
    if (columns != 0 && (columns < 64 || columns > g->cfg.block_size || (columns & (columns - 1)) != 0))
        return fail(SDR_ERR_BAD_ARG, "columns must be 0 or a power of two with 64 <= columns <= block_size");
    if (!g->delivery->on())
        return fail(SDR_ERR_STATE, "rows need bulk delivery (sdr_group_enable_results)");
    for (sdr_bank *b : g->banks)
        if (sdr_listen_pending(b))
            return fail(SDR_ERR_STATE, "a batch waits for its listen half (sdr_group_process_listen)");
    if (g->delivery->parked() > 0)  // (a member batch taken with the old setting's rows)
        return fail(SDR_ERR_STATE, "a batch is half delivered: sdr_group_poll first");
    KeepDevice keep;
    for (sdr_bank *b : g->banks) {
        const int rc = sdr_enable_rows(b, columns);
        if (rc)
            return rc;
    }
    g->delivery->set_rows(columns);
    return SDR_OK;
}

int sdr_group_poll_rows(sdr_group *g, float *rows, int rows_cap, int *n_rows, int64_t *batch_index, int wait)
{
    if (!g || !n_rows || !batch_index || rows_cap < 0 || (!rows && rows_cap > 0))
        return fail(SDR_ERR_BAD_ARG, "null argument");
    KeepDevice keep;
    return g->delivery->poll_rows(rows, rows_cap, n_rows, batch_index, wait != 0);
}

int sdr_group_enable_reports(sdr_group *g, int on)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    // what a member could refuse is checked for all of them first (sdr_group_enable_rows)
    if (!g->delivery->on())
        return fail(SDR_ERR_STATE, "reports need bulk delivery (sdr_group_enable_results)");
    for (sdr_bank *b : g->banks)
        if (sdr_listen_pending(b))
            return fail(SDR_ERR_STATE, "a batch waits for its listen half (sdr_group_process_listen)");
    if (g->delivery->parked() > 0)  // (a member batch taken with the old setting)
        return fail(SDR_ERR_STATE, "a batch is half delivered: sdr_group_poll first");
    KeepDevice keep;
    for (sdr_bank *b : g->banks) {
        const int rc = sdr_enable_reports(b, on);
        if (rc)
            return rc;
    }
    g->delivery->set_reports(on != 0);
    return SDR_OK;
}

int sdr_group_poll_reports(sdr_group *g, sdr_listener_report *out, int cap, int *n_out, int64_t *batch_index, int wait)
{
    if (!g || !n_out || !batch_index || cap < 0 || (!out && cap > 0))
        return fail(SDR_ERR_BAD_ARG, "null argument");
    KeepDevice keep;
    return g->delivery->poll_reports(out, cap, n_out, batch_index, wait != 0);
}

int sdr_group_poll(sdr_group *g, sdr_results *r, int wait)
{
    if (!g || !r)
        return fail(SDR_ERR_BAD_ARG, "null argument");
    if (r->struct_size != (int32_t)sizeof(sdr_results))
        return fail(SDR_ERR_BAD_ARG, "sdr_results.struct_size mismatch (ABI)");
    KeepDevice keep;
    return g->delivery->poll(r, wait != 0);
}

int sdr_group_defer_listen(sdr_group *g, int on)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    for (sdr_bank *b : g->banks)
        if (sdr_listen_pending(b))
            return fail(SDR_ERR_STATE, "a batch waits for its listen half (sdr_group_process_listen)");
    if (on && !g->delivery->on())
        return fail(SDR_ERR_STATE, "deferred listening needs bulk delivery (sdr_group_enable_results)");
    for (sdr_bank *b : g->banks) {
        const int rc = sdr_defer_listen(b, on);
        if (rc)
            return rc;
    }
    return SDR_OK;
}

int sdr_group_poll_peaks(sdr_group *g, sdr_results *r, int wait)
{
    if (!g || !r)
        return fail(SDR_ERR_BAD_ARG, "null argument");
    if (r->struct_size != (int32_t)sizeof(sdr_results))
        return fail(SDR_ERR_BAD_ARG, "sdr_results.struct_size mismatch (ABI)");
    KeepDevice keep;
    return g->delivery->poll_peaks(r, wait != 0);
}

int sdr_group_process_listen(sdr_group *g)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    if (g->failed)
        return fail(SDR_ERR_STATE, "an earlier group call left the members out of step; destroy the group");
    for (sdr_bank *b : g->banks)
        if (!sdr_listen_pending(b))
            return fail(SDR_ERR_STATE, "no group batch waits for its listen half");
    KeepDevice keep;
    for (int m = 0; m < g->rt.n_members; m++) {
        const int rc = sdr_process_listen(g->banks[(size_t)m]);
        if (rc)
            return member_failed(g, rc, m);
    }
    return SDR_OK;
}

int sdr_group_read_drop_counters(sdr_group *g, uint64_t *runes_dropped, uint64_t *edges_dropped)
{
    if (!g)
        return fail(SDR_ERR_BAD_ARG, "null group");
    KeepDevice keep;
    uint64_t runes = 0, edges = 0;
    for (sdr_bank *b : g->banks) {
        uint64_t r = 0, e = 0;
        const int rc = sdr_read_drop_counters(b, &r, &e);
        if (rc)
            return rc;
        runes += r;
        edges += e;
    }
    if (runes_dropped)
        *runes_dropped = runes;
    if (edges_dropped)
        *edges_dropped = edges;
    return SDR_OK;
}

#pragma GCC visibility pop
}  // extern "C"
