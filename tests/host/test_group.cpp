// Host-only test of an sdr_group's bookkeeping (sdrainer_amd/csrc/host/group.h - the code the library runs, not a copy):
// band routing, the frame count of a staged group call, and the merge of the members' deliveries, with synthetic member
// batches behind a fake GroupSource that behaves like sdr_poll (SDR_ERR_WOULD_BLOCK while a member has not finished,
// SDR_ERR_BAD_SIZE with the n_* fields set when a buffer is too small, nothing taken then).  A member batch holds the
// records one bank of the member's bands would deliver; the merge of the members must equal, field by field, what ONE
// bank of all the bands delivers.  Built by tests/test_group_host.py.  No GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "../../sdrainer_amd/csrc/host/group.h"

namespace {

int g_failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            g_failures++;                                                        \
        }                                                                        \
    } while (0)

// One bank's delivery of batch k over `bands` (global band numbers, the bank's local bands in order), in deliver_block's
// order: the records of a band depend on its global number only, their band field is the local index.
struct Batch {
    int64_t batch = 0, first_frame = 0;
    int frames = 0;
    std::vector<sdr_chunk_result> chunks;
    std::vector<sdr_peak> peaks;
    std::vector<sdr_listener_result> listeners;
    std::vector<sdr_edge> edges;
    std::vector<uint32_t> runes, rune_frames;
    uint64_t runes_dropped = 0, edges_dropped = 0;
};

Batch make_batch(const std::vector<int> &bands, int64_t k, int member, bool big)
{
    Batch b;
    b.batch = k;
    b.frames = 250;
    b.first_frame = k * 250;
    b.runes_dropped = (uint64_t)(10 * member + k);
    b.edges_dropped = (uint64_t)(member + 1);
    for (size_t lb = 0; lb < bands.size(); lb++) {
        const int g = bands[lb];
        for (int ch = 0; ch < 2; ch++) {
            sdr_chunk_result c{};
            c.band = (int32_t)lb;
            c.n_peaks = (int32_t)((g + ch + k) % 3);
            c.frame = b.first_frame + 99 + 100 * ch;
            c.first_peak = (int32_t)b.peaks.size();
            c.peaks_found = c.n_peaks + (g == 4 ? 1 : 0);
            for (int i = 0; i < c.n_peaks; i++) {
                sdr_peak p{};
                p.from = 1000 * g + 100 * ch + i;
                p.to = p.from + 5;
                p.signal_bin = p.from + 2;
                p.from_frequency = 7000000 + p.from;
                p.to_frequency = 7000000 + p.to;
                p.signal_frequency = 7000000 + p.signal_bin;
                p.signal_value = 20.5f + (float)g;
                b.peaks.push_back(p);
            }
            b.chunks.push_back(c);
        }
    }
    for (size_t lb = 0; lb < bands.size(); lb++) {
        const int g = bands[lb];
        for (int slot = 0; slot < 3; slot++) {
            const int ne = (((g + slot + k) % 2 == 0) ? slot + 1 : 0) + ((big && g == 3 && slot == 2) ? 400 : 0);
            const int nr = (g + slot) % 3;
            if (!ne && !nr)
                continue;
            sdr_listener_result l{};
            l.band = (int32_t)lb;
            l.listener = slot;
            l.first_edge = (int32_t)b.edges.size();
            l.n_edges = ne;
            l.first_rune = (int32_t)b.runes.size();
            l.n_runes = nr;
            for (int e = 0; e < ne; e++)
                b.edges.push_back(sdr_edge{(uint32_t)(b.first_frame + 10 * g + e), (uint32_t)(e & 1)});
            for (int r = 0; r < nr; r++) {
                b.runes.push_back((uint32_t)('a' + g * 3 + slot + r));
                b.rune_frames.push_back((uint32_t)(b.first_frame + 7 * g + r));
            }
            b.listeners.push_back(l);
        }
    }
    return b;
}

// sdr_poll's contract on a Batch: BAD_SIZE (n_* set, nothing taken) unless everything fits
int deliver(const Batch &b, sdr_results *r)
{
    r->n_frames = b.frames;
    r->batch_index = b.batch;
    r->first_frame = b.first_frame;
    r->n_chunks = (int32_t)b.chunks.size();
    r->n_peaks = (int32_t)b.peaks.size();
    r->n_listeners = (int32_t)b.listeners.size();
    r->n_edges = (int32_t)b.edges.size();
    r->n_runes = (int32_t)b.runes.size();
    r->runes_dropped = b.runes_dropped;
    r->edges_dropped = b.edges_dropped;
    if (r->n_chunks > r->chunks_cap || r->n_peaks > r->peaks_cap || r->n_listeners > r->listeners_cap || r->n_edges > r->edges_cap ||
        r->n_runes > r->runes_cap)
        return SDR_ERR_BAD_SIZE;
    std::copy(b.chunks.begin(), b.chunks.end(), r->chunks);
    std::copy(b.peaks.begin(), b.peaks.end(), r->peaks);
    std::copy(b.listeners.begin(), b.listeners.end(), r->listeners);
    std::copy(b.edges.begin(), b.edges.end(), r->edges);
    std::copy(b.runes.begin(), b.runes.end(), r->runes);
    std::copy(b.rune_frames.begin(), b.rune_frames.end(), r->rune_frames);
    return SDR_OK;
}

struct FakeMembers final : host::GroupSource {
    std::vector<std::deque<Batch>> finished;  // per member: batches finished and not yet taken
    std::vector<int> polls, bad_sizes;
    std::string last;
    explicit FakeMembers(int m) : finished((size_t)m), polls((size_t)m), bad_sizes((size_t)m) {}
    int poll(int m, sdr_results *r, bool) override
    {
        polls[(size_t)m]++;
        auto &q = finished[(size_t)m];
        if (q.empty())
            return report(SDR_ERR_WOULD_BLOCK, "member has not finished");
        const int rc = deliver(q.front(), r);
        if (rc == SDR_OK)
            q.pop_front();
        else
            bad_sizes[(size_t)m]++;
        return rc;
    }
    int poll_peaks(int m, sdr_results *r, bool wait) override
    {
        auto &q = finished[(size_t)m];
        if (q.empty())
            return report(SDR_ERR_WOULD_BLOCK, "member has not finished");
        Batch b = q.front();  // (the batch stays undelivered; the listen half is not there yet)
        b.listeners.clear();
        b.edges.clear();
        b.runes.clear();
        b.rune_frames.clear();
        (void)wait;
        return deliver(b, r);
    }
    int report(int code, const char *msg) override
    {
        last = msg;
        return code;
    }
};

std::vector<int> bands_of(const host::GroupRouting &rt, int m)
{
    std::vector<int> v;
    for (int g = 0; g < rt.n_bands; g++)
        if (rt.member_of(g) == m)
            v.push_back(g);
    return v;
}

// caller-side buffers
struct Out {
    std::vector<sdr_chunk_result> chunks;
    std::vector<sdr_peak> peaks;
    std::vector<sdr_listener_result> listeners;
    std::vector<sdr_edge> edges;
    std::vector<uint32_t> runes, rune_frames;
    sdr_results r{};
    explicit Out(int cap)
        : chunks((size_t)cap), peaks((size_t)cap), listeners((size_t)cap), edges((size_t)cap), runes((size_t)cap), rune_frames((size_t)cap)
    {
        r.struct_size = (int32_t)sizeof r;
        r.chunks = chunks.data();
        r.chunks_cap = cap;
        r.peaks = peaks.data();
        r.peaks_cap = cap;
        r.listeners = listeners.data();
        r.listeners_cap = cap;
        r.edges = edges.data();
        r.edges_cap = cap;
        r.runes = runes.data();
        r.rune_frames = rune_frames.data();
        r.runes_cap = cap;
    }
};

// delivered == one bank's batch over all bands, field by field (bytes: the records have no padding)
bool equals_one_bank(const Out &o, const Batch &want, const Batch &drops)
{
    const sdr_results &r = o.r;
    bool ok = r.batch_index == want.batch && r.first_frame == want.first_frame && r.n_frames == want.frames &&
              r.n_chunks == (int32_t)want.chunks.size() && r.n_peaks == (int32_t)want.peaks.size() &&
              r.n_listeners == (int32_t)want.listeners.size() && r.n_edges == (int32_t)want.edges.size() &&
              r.n_runes == (int32_t)want.runes.size() && r.runes_dropped == drops.runes_dropped && r.edges_dropped == drops.edges_dropped;
    if (!ok)
        return false;
    auto same = [](const void *a, const void *b, size_t bytes) { return bytes == 0 || std::memcmp(a, b, bytes) == 0; };
    return same(o.chunks.data(), want.chunks.data(), want.chunks.size() * sizeof(sdr_chunk_result)) &&
           same(o.peaks.data(), want.peaks.data(), want.peaks.size() * sizeof(sdr_peak)) &&
           same(o.listeners.data(), want.listeners.data(), want.listeners.size() * sizeof(sdr_listener_result)) &&
           same(o.edges.data(), want.edges.data(), want.edges.size() * sizeof(sdr_edge)) &&
           same(o.runes.data(), want.runes.data(), want.runes.size() * sizeof(uint32_t)) &&
           same(o.rune_frames.data(), want.rune_frames.data(), want.rune_frames.size() * sizeof(uint32_t));
}

Batch summed_drops(int n_members, int64_t k)
{
    Batch d;
    for (int m = 0; m < n_members; m++) {
        d.runes_dropped += (uint64_t)(10 * m + k);
        d.edges_dropped += (uint64_t)(m + 1);
    }
    return d;
}

void test_routing()
{
    host::GroupRouting r2{5, 2}, r3{5, 3};
    CHECK(r2.valid() && r3.valid());
    CHECK(r2.bands_of(0) == 3 && r2.bands_of(1) == 2);
    CHECK(r3.bands_of(0) == 2 && r3.bands_of(1) == 2 && r3.bands_of(2) == 1);
    const int m2[] = {0, 1, 0, 1, 0}, l2[] = {0, 0, 1, 1, 2};
    const int m3[] = {0, 1, 2, 0, 1}, l3[] = {0, 0, 0, 1, 1};
    for (int b = 0; b < 5; b++) {
        CHECK(r2.member_of(b) == m2[b] && r2.local_of(b) == l2[b] && r2.global_of(m2[b], l2[b]) == b);
        CHECK(r3.member_of(b) == m3[b] && r3.local_of(b) == l3[b] && r3.global_of(m3[b], l3[b]) == b);
    }
    CHECK(!(host::GroupRouting{2, 3}.valid()) && !(host::GroupRouting{4, 0}.valid()) && (host::GroupRouting{3, 3}.valid()));
    std::printf("routing ok\n");
}

void test_frames()
{
    CHECK(host::group_frames({300, 120, 500, 250, 999}, 1024, 1024) == 120);
    CHECK(host::group_frames({300, 0, 500, 250, 999}, 1024, 1024) == 0);  // a band with nothing staged holds the group
    CHECK(host::group_frames({300, 120, 500}, 100, 1024) == 100);         // _limit
    CHECK(host::group_frames({300, 320, 500}, 1024, 256) == 256);         // capacity
    CHECK(host::group_frames({300, 320, 500}, -5, 256) == 0);
    std::printf("frames ok\n");
}

// several batches, members finishing in a different order each time; one member's batch outgrows the group's buffers
void test_merge(int n_members)
{
    host::GroupRouting rt{5, n_members};
    FakeMembers src(n_members);
    host::GroupDelivery d(&src, rt);
    Out out(4096);
    CHECK(d.poll(&out.r, false) == SDR_ERR_STATE);  // delivery off
    d.reset(true);
    const std::vector<int> all = {0, 1, 2, 3, 4};
    for (int64_t k = 0; k < 4; k++) {
        const bool big = k == 2;
        for (int m = 0; m < n_members; m++)
            src.finished[(size_t)m].push_back(make_batch(bands_of(rt, m), k, m, big));
        CHECK(d.poll(&out.r, false) == SDR_OK);
        CHECK(equals_one_bank(out, make_batch(all, k, 0, big), summed_drops(n_members, k)));
        CHECK(d.parked() == 0);
    }
    CHECK(d.poll(&out.r, false) == SDR_ERR_WOULD_BLOCK);
    int grown = 0;
    for (int v : src.bad_sizes)
        grown += v;
    CHECK(grown == 1);  // the big batch: BAD_SIZE from its member once, then the group's buffers were large enough
    std::printf("merge%d ok\n", n_members);
}

void test_offsets()
{
    host::GroupRouting rt{5, 2};
    FakeMembers src(2);
    host::GroupDelivery d(&src, rt);
    d.reset(true);
    Out out(4096);
    for (int m = 0; m < 2; m++)
        src.finished[(size_t)m].push_back(make_batch(bands_of(rt, m), 1, m, false));
    CHECK(d.poll(&out.r, true) == SDR_OK);
    const sdr_results &r = out.r;
    int pi = 0, ei = 0, ri = 0, prev_band = -1;
    for (int c = 0; c < r.n_chunks; c++) {
        CHECK(out.chunks[(size_t)c].first_peak == pi && out.chunks[(size_t)c].band >= prev_band);
        for (int i = 0; i < out.chunks[(size_t)c].n_peaks; i++)
            CHECK(out.peaks[(size_t)(pi + i)].from / 1000 == out.chunks[(size_t)c].band);  // a band's peaks follow its chunk
        prev_band = out.chunks[(size_t)c].band;
        pi += out.chunks[(size_t)c].n_peaks;
    }
    CHECK(pi == r.n_peaks);
    prev_band = -1;
    for (int l = 0; l < r.n_listeners; l++) {
        const sdr_listener_result &x = out.listeners[(size_t)l];
        CHECK(x.first_edge == ei && x.first_rune == ri && x.band >= prev_band);
        for (int e = 0; e < x.n_edges; e++)
            CHECK(out.edges[(size_t)(ei + e)].frame == (uint32_t)(r.first_frame + 10 * x.band + e));
        for (int k = 0; k < x.n_runes; k++)
            CHECK(out.runes[(size_t)(ri + k)] == (uint32_t)('a' + x.band * 3 + x.listener + k));
        prev_band = x.band;
        ei += x.n_edges;
        ri += x.n_runes;
    }
    CHECK(ei == r.n_edges && ri == r.n_runes);
    CHECK(r.runes_dropped == 0 + 1 + 10 + 1 && r.edges_dropped == 1 + 2);
    std::printf("offsets ok\n");
}

// the caller's buffers are too small: nothing is delivered, the n_* fields say what is needed, the members' batches stay
// parked in the group, and the retry delivers the same batch whole
void test_bad_size()
{
    host::GroupRouting rt{5, 2};
    FakeMembers src(2);
    host::GroupDelivery d(&src, rt);
    d.reset(true);
    const std::vector<int> all = {0, 1, 2, 3, 4};
    for (int m = 0; m < 2; m++) {
        src.finished[(size_t)m].push_back(make_batch(bands_of(rt, m), 0, m, false));
        src.finished[(size_t)m].push_back(make_batch(bands_of(rt, m), 1, m, false));
    }
    const Batch want = make_batch(all, 0, 0, false);
    Out small(4);
    std::vector<sdr_chunk_result> before(small.chunks);
    CHECK(d.poll(&small.r, false) == SDR_ERR_BAD_SIZE);
    CHECK(small.r.n_chunks == (int32_t)want.chunks.size() && small.r.n_peaks == (int32_t)want.peaks.size() &&
          small.r.n_listeners == (int32_t)want.listeners.size() && small.r.n_edges == (int32_t)want.edges.size() &&
          small.r.n_runes == (int32_t)want.runes.size() && small.r.batch_index == 0);
    CHECK(std::memcmp(before.data(), small.chunks.data(), before.size() * sizeof(sdr_chunk_result)) == 0);  // nothing written
    CHECK(d.parked() == 2 && src.finished[0].size() == 1 && src.finished[1].size() == 1);
    CHECK(d.poll(&small.r, false) == SDR_ERR_BAD_SIZE && d.parked() == 2);
    Out out(4096);
    CHECK(d.poll(&out.r, false) == SDR_OK);
    CHECK(equals_one_bank(out, want, summed_drops(2, 0)));
    CHECK(d.parked() == 0);
    CHECK(d.poll(&out.r, false) == SDR_OK);
    CHECK(equals_one_bank(out, make_batch(all, 1, 0, false), summed_drops(2, 1)));
    std::printf("bad_size ok\n");
}

// wait = 0 while one member is behind: WOULD_BLOCK, the other members' batches parked; once it finishes, the whole batch
void test_would_block()
{
    host::GroupRouting rt{5, 3};
    FakeMembers src(3);
    host::GroupDelivery d(&src, rt);
    d.reset(true);
    const std::vector<int> all = {0, 1, 2, 3, 4};
    Out out(4096);
    src.finished[0].push_back(make_batch(bands_of(rt, 0), 0, 0, false));
    src.finished[2].push_back(make_batch(bands_of(rt, 2), 0, 2, false));
    CHECK(d.poll(&out.r, false) == SDR_ERR_WOULD_BLOCK);
    CHECK(d.parked() == 1);  // member 0 taken and parked; member 1 behind; member 2 not reached yet
    CHECK(d.poll(&out.r, false) == SDR_ERR_WOULD_BLOCK && d.parked() == 1);
    src.finished[0].push_back(make_batch(bands_of(rt, 0), 1, 0, false));  // member 0 runs ahead
    CHECK(d.poll(&out.r, false) == SDR_ERR_WOULD_BLOCK && d.parked() == 1 && src.finished[0].size() == 1);
    src.finished[1].push_back(make_batch(bands_of(rt, 1), 0, 1, false));
    CHECK(d.poll(&out.r, false) == SDR_OK);
    CHECK(equals_one_bank(out, make_batch(all, 0, 0, false), summed_drops(3, 0)));
    CHECK(d.parked() == 0);
    CHECK(d.poll(&out.r, false) == SDR_ERR_WOULD_BLOCK);  // batch 1: members 1 and 2 behind
    src.finished[1].push_back(make_batch(bands_of(rt, 1), 1, 1, false));
    src.finished[2].push_back(make_batch(bands_of(rt, 2), 1, 2, false));
    CHECK(d.poll(&out.r, false) == SDR_OK);
    CHECK(equals_one_bank(out, make_batch(all, 1, 0, false), summed_drops(3, 1)));
    // the mode goes, and what was parked goes with it
    src.finished[0].push_back(make_batch(bands_of(rt, 0), 2, 0, false));
    CHECK(d.poll(&out.r, false) == SDR_ERR_WOULD_BLOCK && d.parked() == 1);
    d.reset(false);
    CHECK(d.parked() == 0 && d.poll(&out.r, false) == SDR_ERR_STATE);
    std::printf("would_block ok\n");
}

// members that delivered different batches: SDR_ERR_STATE, nothing delivered
void test_out_of_step()
{
    host::GroupRouting rt{4, 2};
    FakeMembers src(2);
    host::GroupDelivery d(&src, rt);
    d.reset(true);
    Out out(4096);
    src.finished[0].push_back(make_batch(bands_of(rt, 0), 0, 0, false));
    Batch other = make_batch(bands_of(rt, 1), 0, 1, false);
    other.first_frame += 1;
    src.finished[1].push_back(other);
    CHECK(d.poll(&out.r, false) == SDR_ERR_STATE);
    CHECK(src.last.find("different batches") != std::string::npos);
    std::printf("out_of_step ok\n");
}

void test_poll_peaks()
{
    host::GroupRouting rt{5, 2};
    FakeMembers src(2);
    host::GroupDelivery d(&src, rt);
    d.reset(true);
    Out out(4096);
    src.finished[0].push_back(make_batch(bands_of(rt, 0), 0, 0, false));
    CHECK(d.poll_peaks(&out.r, false) == SDR_ERR_WOULD_BLOCK);
    src.finished[1].push_back(make_batch(bands_of(rt, 1), 0, 1, false));
    CHECK(d.poll_peaks(&out.r, false) == SDR_OK);
    Batch want = make_batch({0, 1, 2, 3, 4}, 0, 0, false);
    want.listeners.clear();
    want.edges.clear();
    want.runes.clear();
    want.rune_frames.clear();
    CHECK(equals_one_bank(out, want, summed_drops(2, 0)));
    CHECK(d.parked() == 0 && src.finished[0].size() == 1 && src.finished[1].size() == 1);  // nothing taken
    std::printf("poll_peaks ok\n");
}

}  // namespace

int main()
{
    test_routing();
    test_frames();
    test_merge(2);
    test_merge(3);
    test_offsets();
    test_bad_size();
    test_would_block();
    test_out_of_step();
    test_poll_peaks();
    return g_failures ? 1 : 0;
}
