// host/group.h — the bookkeeping of an sdr_group (include/sdrainer_hip.h): several banks, one per member device, that
// a host drives as ONE bank of n_bands bands.  Which member and local band a band lives on, how many frames a staged
// process call consumes, and how the members' deliveries of one batch become one delivery in exactly the order a
// single bank of n_bands bands would give (deliver_block in capi_results.hip) - with a member batch that was already
// taken from its bank parked here until the whole batch goes out.
//
// Pure C++: the members' sdr_poll / sdr_poll_peaks sit behind GroupSource, so the same code that libsdrainer_hip.so
// runs (capi_group.hip) is driven by tests/host/test_group.cpp with synthetic member results and no GPU.
//
// Rules:
//  * band b lives on member b % n_members as local band b / n_members (sharding.bands_of_rank);
//  * a group batch k is delivered only once every member has delivered its batch k, whole, exactly once and in order;
//    batch_index, first_frame and n_frames of the member batches must agree (SDR_ERR_STATE otherwise);
//  * the parked member batches belong to the consumer: poll() and reset() serialise on `mu_`.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../../include/sdrainer_hip.h"

namespace host {

struct GroupRouting {
    int n_bands = 0, n_members = 0;
    int member_of(int band) const { return band % n_members; }
    int local_of(int band) const { return band / n_members; }
    int global_of(int member, int local) const { return local * n_members + member; }
    int bands_of(int member) const { return (n_bands - member + n_members - 1) / n_members; }
    bool valid() const { return n_members >= 1 && n_bands >= n_members; }
};

// Frames one group process call consumes per band: the minimum of what every band of the group has staged, as one bank
// takes the minimum over its own bands (sdr_process_staged_limit), capped by max_frames and the batch capacity.
inline int group_frames(const std::vector<int> &staged, int max_frames, int max_batch_frames)
{
    int n = std::min(max_batch_frames, std::max(max_frames, 0));
    for (int v : staged)
        n = std::min(n, std::max(v, 0));
    return n;
}

// One member's batch in buffers of the group's own (grown to what the bank says it needs).
struct MemberBatch {
    sdr_results r{};
    std::vector<sdr_chunk_result> chunks = std::vector<sdr_chunk_result>(16);
    std::vector<sdr_peak> peaks = std::vector<sdr_peak>(64);
    std::vector<sdr_listener_result> listeners = std::vector<sdr_listener_result>(16);
    std::vector<sdr_edge> edges = std::vector<sdr_edge>(256);
    std::vector<uint32_t> runes = std::vector<uint32_t>(256), rune_frames = std::vector<uint32_t>(256);
    bool held = false;  // r describes a batch taken from the member's bank and not delivered yet
    // the batch's waterfall rows (sdr_group_enable_rows), peeked from the bank right before the batch was taken from it
    std::vector<float> rows;
    int n_rows = 0;
    // ... and its listener reports (sdr_group_enable_reports), peeked the same way; bands are the member's local ones
    std::vector<sdr_listener_report> reports;
    int n_reports = 0;

    void bind()
    {
        r.struct_size = (int32_t)sizeof(sdr_results);
        r.chunks = chunks.data();
        r.chunks_cap = (int32_t)chunks.size();
        r.peaks = peaks.data();
        r.peaks_cap = (int32_t)peaks.size();
        r.listeners = listeners.data();
        r.listeners_cap = (int32_t)listeners.size();
        r.edges = edges.data();
        r.edges_cap = (int32_t)edges.size();
        r.runes = runes.data();
        r.rune_frames = rune_frames.data();
        r.runes_cap = (int32_t)runes.size();
    }
    // after SDR_ERR_BAD_SIZE: r's n_* fields say what is needed
    void grow()
    {
        auto at_least = [](auto &v, int32_t n) {
            if ((size_t)std::max(n, 0) > v.size())
                v.resize((size_t)n + (size_t)n / 2);
        };
        at_least(chunks, r.n_chunks);
        at_least(peaks, r.n_peaks);
        at_least(listeners, r.n_listeners);
        at_least(edges, r.n_edges);
        at_least(runes, r.n_runes);
        at_least(rune_frames, r.n_runes);
    }
};

struct GroupSource {
    virtual ~GroupSource() = default;
    // a member's sdr_poll / sdr_poll_peaks into r
    virtual int poll(int member, sdr_results *r, bool wait) = 0;
    virtual int poll_peaks(int member, sdr_results *r, bool wait) = 0;
    // a member's sdr_poll_rows (a source without rows delivers none)
    virtual int poll_rows(int, float *, int, int *n_rows, int64_t *batch_index, bool)
    {
        *n_rows = 0;
        *batch_index = -1;
        return SDR_OK;
    }
    // a member's sdr_poll_reports (a source without reports delivers none)
    virtual int poll_reports(int, sdr_listener_report *, int, int *n_out, int64_t *batch_index, bool)
    {
        *n_out = 0;
        *batch_index = -1;
        return SDR_OK;
    }
    virtual int report(int code, const char *msg) = 0;  // records the message for sdr_last_error(), returns code
};

// The members' batches (all of the same batch) into the caller's buffers with global band numbers: chunks by band, then
// chunk; listeners by band, then slot; first_peak / first_edge / first_rune renumbered; drop counters summed.  Nothing
// is written to the buffers unless all of it fits (SDR_ERR_BAD_SIZE with the n_* fields set, as deliver_block does).
inline int merge_batches(const GroupRouting &rt, const std::vector<MemberBatch> &mb, sdr_results *out, GroupSource *src)
{
    const int M = rt.n_members;
    const sdr_results &r0 = mb[0].r;
    int64_t n_chunks = 0, n_peaks = 0, n_listeners = 0, n_edges = 0, n_runes = 0;
    uint64_t runes_dropped = 0, edges_dropped = 0;
    for (int m = 0; m < M; m++) {
        const sdr_results &r = mb[(size_t)m].r;
        if (r.batch_index != r0.batch_index || r.first_frame != r0.first_frame || r.n_frames != r0.n_frames)
            return src->report(SDR_ERR_STATE, "sdr_group_poll: the members delivered different batches (out of step)");
        const MemberBatch &b = mb[(size_t)m];
        if (r.n_chunks < 0 || r.n_peaks < 0 || r.n_listeners < 0 || r.n_edges < 0 || r.n_runes < 0 ||
            (size_t)r.n_chunks > b.chunks.size() || (size_t)r.n_peaks > b.peaks.size() || (size_t)r.n_listeners > b.listeners.size() ||
            (size_t)r.n_edges > b.edges.size() || (size_t)r.n_runes > b.runes.size() || (size_t)r.n_runes > b.rune_frames.size())
            return src->report(SDR_ERR_STATE, "sdr_group_poll: a member delivered counts its buffers cannot hold");
        n_chunks += r.n_chunks;
        n_peaks += r.n_peaks;
        n_listeners += r.n_listeners;
        n_edges += r.n_edges;
        n_runes += r.n_runes;
        runes_dropped += r.runes_dropped;
        edges_dropped += r.edges_dropped;
    }
    const bool fits = n_chunks <= out->chunks_cap && n_peaks <= out->peaks_cap && n_listeners <= out->listeners_cap &&
                      n_edges <= out->edges_cap && n_runes <= out->runes_cap && (n_chunks == 0 || out->chunks) &&
                      (n_peaks == 0 || out->peaks) && (n_listeners == 0 || out->listeners) && (n_edges == 0 || out->edges) &&
                      (n_runes == 0 || (out->runes && out->rune_frames));
    out->n_chunks = (int32_t)n_chunks;
    out->n_peaks = (int32_t)n_peaks;
    out->n_listeners = (int32_t)n_listeners;
    out->n_edges = (int32_t)n_edges;
    out->n_runes = (int32_t)n_runes;
    out->n_frames = r0.n_frames;
    out->batch_index = r0.batch_index;
    out->first_frame = r0.first_frame;
    out->runes_dropped = runes_dropped;
    out->edges_dropped = edges_dropped;
    if (!fits)
        return src->report(SDR_ERR_BAD_SIZE, "sdr_group_poll: a result buffer is too small (the n_* fields say what is needed)");
    // a bank lists its records by local band, ascending: one cursor per member walks them as the global bands come up
    std::vector<int> ccur((size_t)M, 0), lcur((size_t)M, 0);
    int ci = 0, pi = 0, li = 0, ei = 0, ri = 0;
    for (int g = 0; g < rt.n_bands; g++) {
        const int m = rt.member_of(g), lb = rt.local_of(g);
        const MemberBatch &b = mb[(size_t)m];
        for (int &k = ccur[(size_t)m]; k < b.r.n_chunks && b.chunks[(size_t)k].band == lb; k++) {
            const sdr_chunk_result &c = b.chunks[(size_t)k];
            if (c.n_peaks < 0 || c.first_peak < 0 || (int64_t)c.first_peak + c.n_peaks > b.r.n_peaks)
                return src->report(SDR_ERR_STATE, "sdr_group_poll: a member's chunk points outside its peaks");
            sdr_chunk_result &o = out->chunks[ci++];
            o = c;
            o.band = g;
            o.first_peak = pi;
            std::copy_n(b.peaks.begin() + c.first_peak, c.n_peaks, out->peaks + pi);
            pi += c.n_peaks;
        }
    }
    for (int g = 0; g < rt.n_bands; g++) {
        const int m = rt.member_of(g), lb = rt.local_of(g);
        const MemberBatch &b = mb[(size_t)m];
        for (int &k = lcur[(size_t)m]; k < b.r.n_listeners && b.listeners[(size_t)k].band == lb; k++) {
            const sdr_listener_result &l = b.listeners[(size_t)k];
            if (l.n_edges < 0 || l.first_edge < 0 || (int64_t)l.first_edge + l.n_edges > b.r.n_edges || l.n_runes < 0 ||
                l.first_rune < 0 || (int64_t)l.first_rune + l.n_runes > b.r.n_runes)
                return src->report(SDR_ERR_STATE, "sdr_group_poll: a member's listener points outside its edges / runes");
            sdr_listener_result &o = out->listeners[li++];
            o = l;
            o.band = g;
            o.first_edge = ei;
            o.first_rune = ri;
            std::copy_n(b.edges.begin() + l.first_edge, l.n_edges, out->edges + ei);
            std::copy_n(b.runes.begin() + l.first_rune, l.n_runes, out->runes + ri);
            std::copy_n(b.rune_frames.begin() + l.first_rune, l.n_runes, out->rune_frames + ri);
            ei += l.n_edges;
            ri += l.n_runes;
        }
    }
    for (int m = 0; m < M; m++)
        if (ccur[(size_t)m] != mb[(size_t)m].r.n_chunks || lcur[(size_t)m] != mb[(size_t)m].r.n_listeners)
            return src->report(SDR_ERR_STATE, "sdr_group_poll: a member's records are not ordered by band");
    return SDR_OK;
}

class GroupDelivery {
public:
    GroupDelivery(GroupSource *src, GroupRouting rt) : src_(src), rt_(rt), parked_((size_t)rt.n_members), peeked_((size_t)rt.n_members) {}

    // sdr_group_enable_results: member batches parked here go with the mode, as the banks discard theirs
    void reset(bool on)
    {
        std::lock_guard<std::mutex> g(mu_);
        on_ = on;
        for (auto &p : parked_)
            p.held = false;
    }
    bool on()
    {
        std::lock_guard<std::mutex> g(mu_);
        return on_;
    }
    // sdr_group_enable_rows: from now on a member batch is taken together with its rows, `columns` values each (0: none)
    void set_rows(int columns)
    {
        std::lock_guard<std::mutex> g(mu_);
        row_columns_ = columns;
    }
    // sdr_group_enable_reports: from now on a member batch is taken together with its listener reports
    void set_reports(bool on)
    {
        std::lock_guard<std::mutex> g(mu_);
        reports_on_ = on;
    }

    // The oldest batch every member has finished, merged.  A member batch taken from its bank stays parked here through
    // SDR_ERR_WOULD_BLOCK (another member is behind), SDR_ERR_BAD_SIZE (the caller's buffers) and SDR_ERR_STATE, and
    // the next call delivers it whole.
    int poll(sdr_results *out, bool wait)
    {
        std::lock_guard<std::mutex> g(mu_);
        if (!on_)
            return src_->report(SDR_ERR_STATE, "bulk delivery is off (sdr_group_enable_results)");
        for (int m = 0; m < rt_.n_members; m++) {
            MemberBatch &p = parked_[(size_t)m];
            if (p.held)
                continue;
            const int rc = take(m, p, wait, false);
            if (rc != SDR_OK)
                return rc;
            p.held = true;
        }
        const int rc = merge_batches(rt_, parked_, out, src_);
        if (rc == SDR_OK)
            for (auto &p : parked_)
                p.held = false;
        return rc;
    }

    // sdr_group_poll_rows: the rows of the oldest batch every member has finished, in the order poll() gives its chunks
    // (global band, then chunk).  A peek for the caller - the next poll() delivers the same batch - but the member batches
    // ARE taken from their banks (rows first, then the batch) and parked here, as poll() parks them: a bank hands out the
    // rows of its oldest undelivered batch only.
    int poll_rows(float *rows, int rows_cap, int *n_rows, int64_t *batch_index, bool wait)
    {
        std::lock_guard<std::mutex> g(mu_);
        if (!on_)
            return src_->report(SDR_ERR_STATE, "bulk delivery is off (sdr_group_enable_results)");
        for (int m = 0; m < rt_.n_members; m++) {
            MemberBatch &p = parked_[(size_t)m];
            if (p.held)
                continue;
            const int rc = take(m, p, wait, false);
            if (rc != SDR_OK)
                return rc;
            p.held = true;
        }
        // every member completed the same cumulations: rows per band, the same on all members that have any
        int total = 0, per_band = -1, columns = 0;
        for (int m = 0; m < rt_.n_members; m++) {
            const MemberBatch &p = parked_[(size_t)m];
            if (p.r.batch_index != parked_[0].r.batch_index)
                return src_->report(SDR_ERR_STATE, "sdr_group_poll_rows: the members delivered different batches (out of step)");
            const int bands = rt_.bands_of(m);
            if (p.n_rows % bands != 0 || (per_band >= 0 && p.n_rows / bands != per_band))
                return src_->report(SDR_ERR_STATE, "sdr_group_poll_rows: the members' row counts disagree");
            per_band = p.n_rows / bands;
            if (p.n_rows > 0)
                columns = (int)(p.rows.size() / (size_t)p.n_rows);
            total += p.n_rows;
        }
        *n_rows = total;
        *batch_index = parked_[0].r.batch_index;
        if (total == 0)
            return SDR_OK;
        if (total > rows_cap || !rows)
            return src_->report(SDR_ERR_BAD_SIZE, "sdr_group_poll_rows: rows_cap is too small (*n_rows says what is needed)");
        float *dst = rows;
        for (int gb = 0; gb < rt_.n_bands; gb++) {
            const MemberBatch &p = parked_[(size_t)rt_.member_of(gb)];
            const float *src = p.rows.data() + (size_t)rt_.local_of(gb) * (size_t)per_band * (size_t)columns;
            dst = std::copy_n(src, (size_t)per_band * (size_t)columns, dst);
        }
        return SDR_OK;
    }

    // sdr_group_poll_reports: the listener reports of the oldest batch every member has finished, in one bank's order
    // (global band, then listener id) with global band numbers.  A peek for the caller, with the member batches taken and
    // parked here as poll_rows takes them.
    int poll_reports(sdr_listener_report *out, int cap, int *n_out, int64_t *batch_index, bool wait)
    {
        std::lock_guard<std::mutex> g(mu_);
        if (!on_)
            return src_->report(SDR_ERR_STATE, "bulk delivery is off (sdr_group_enable_results)");
        for (int m = 0; m < rt_.n_members; m++) {
            MemberBatch &p = parked_[(size_t)m];
            if (p.held)
                continue;
            const int rc = take(m, p, wait, false);
            if (rc != SDR_OK)
                return rc;
            p.held = true;
        }
        int total = 0;
        for (int m = 0; m < rt_.n_members; m++) {
            if (parked_[(size_t)m].r.batch_index != parked_[0].r.batch_index)
                return src_->report(SDR_ERR_STATE, "sdr_group_poll_reports: the members delivered different batches (out of step)");
            total += parked_[(size_t)m].n_reports;
        }
        *n_out = total;
        *batch_index = parked_[0].r.batch_index;
        if (total == 0)
            return SDR_OK;
        if (total > cap || !out)
            return src_->report(SDR_ERR_BAD_SIZE, "sdr_group_poll_reports: cap is too small (*n_out says what is needed)");
        // a member's records are sorted by local band, then listener: global band gb's are one run of them
        sdr_listener_report *dst = out;
        for (int gb = 0; gb < rt_.n_bands; gb++) {
            const MemberBatch &p = parked_[(size_t)rt_.member_of(gb)];
            const int local = rt_.local_of(gb);
            for (int i = 0; i < p.n_reports; i++)
                if (p.reports[(size_t)i].band == local) {
                    *dst = p.reports[(size_t)i];
                    dst->band = gb;
                    dst++;
                }
        }
        return SDR_OK;
    }

    // sdr_group_poll_peaks: the chunks and peaks of the batch that waits for its listen half.  The banks keep that batch
    // undelivered, so nothing is parked: the members are read into scratch buffers of their own (the producer's, not the
    // consumer's).
    int poll_peaks(sdr_results *out, bool wait)
    {
        std::lock_guard<std::mutex> g(peek_mu_);
        for (int m = 0; m < rt_.n_members; m++) {
            const int rc = take(m, peeked_[(size_t)m], wait, true);
            if (rc != SDR_OK)
                return rc;
        }
        return merge_batches(rt_, peeked_, out, src_);
    }

    // (tests)
    int parked()
    {
        std::lock_guard<std::mutex> g(mu_);
        int n = 0;
        for (auto &p : parked_)
            n += p.held ? 1 : 0;
        return n;
    }

private:
    int take(int m, MemberBatch &p, bool wait, bool peaks)
    {
        // the rows go first: once the batch itself is taken the bank's oldest undelivered batch is the next one
        if (!peaks) {
            p.n_rows = 0;
            p.rows.clear();
            int64_t batch = -1;
            for (int attempt = 0; row_columns_ > 0 && attempt < 2; attempt++) {
                int n = 0;
                const int cap = (int)(p.rows.size() / (size_t)row_columns_);
                const int rc = src_->poll_rows(m, p.rows.data(), cap, &n, &batch, wait);
                if (rc == SDR_ERR_BAD_SIZE && attempt == 0) {
                    p.rows.resize((size_t)n * (size_t)row_columns_);
                    continue;
                }
                if (rc != SDR_OK)
                    return rc;
                p.n_rows = n;
                p.rows.resize((size_t)n * (size_t)row_columns_);
                break;
            }
        }
        if (!peaks) {
            p.n_reports = 0;
            int64_t batch = -1;
            for (int attempt = 0; reports_on_ && attempt < 2; attempt++) {
                int n = 0;
                const int rc = src_->poll_reports(m, p.reports.data(), (int)p.reports.size(), &n, &batch, wait);
                if (rc == SDR_ERR_BAD_SIZE && attempt == 0) {
                    p.reports.resize((size_t)n);
                    continue;
                }
                if (rc != SDR_OK)
                    return rc;
                p.n_reports = n;
                break;
            }
        }
        for (int attempt = 0; attempt < 4; attempt++) {
            p.bind();
            const int rc = peaks ? src_->poll_peaks(m, &p.r, wait) : src_->poll(m, &p.r, wait);
            if (rc != SDR_ERR_BAD_SIZE)
                return rc;
            p.grow();  // (the member delivered nothing: the same batch comes again)
        }
        return src_->report(SDR_ERR_STATE, "sdr_group_poll: a member's batch keeps outgrowing the group's buffers");
    }

    GroupSource *src_;
    GroupRouting rt_;
    std::mutex mu_, peek_mu_;
    bool on_ = false;
    int row_columns_ = 0;
    bool reports_on_ = false;
    std::vector<MemberBatch> parked_, peeked_;
};

}  // namespace host
