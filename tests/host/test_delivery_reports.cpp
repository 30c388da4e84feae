// Host-only model test of bulk delivery with a report block (sdrainer_amd/csrc/host/delivery.h - the code the library runs
// behind sdr_poll_reports, not a copy): fake events, a block and a report block per set, filled the way k_listen_report
// fills it - one record per listener slot, listener = -1 where the slot is not active.  Checked: peek_reports looks at the
// batch the next poll() hands out and leaves it undelivered; it blocks exactly where poll() would - a batch whose listen
// half is still to come shows nothing; a buffer too small is refused with the count needed and the retry delivers; the
// records arrive by band, then listener id, the inactive slots left out; a batch parked on the host - ring reuse, the end
// of graph mode - takes its reports with it; a batch processed with reports off, or without an active listener, delivers
// none.  Built plain and with the sanitizers by tests/test_delivery_reports.py.  No GPU, no HIP.
//
// Scenarios:
//   order      publish, peek (not finished / finished), BAD_SIZE and retry, poll, a batch with reports off, one without listeners
//   park       ten batches, nobody polls: the first four are parked with their reports when their sets are reused
//   deferred   a batch published without its listen half: no reports until the listen half is enqueued and has finished
//   graph      graph sets, then graph_end: what was not polled is parked with its reports; eager batches follow
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../sdrainer_amd/csrc/host/delivery.h"

namespace {

constexpr int RING = 6, SPAN = 12, BANDS = 2, STRIDE = 5;  // five listener slots per band
constexpr size_t BLOCK = 16;

struct FakeEvent {
    std::atomic<int64_t> done{-1}, want{-1};
};

struct Out {
    int64_t batch = -1, stamp = -1;
};

std::string g_err;
int g_failed = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d %s (%s)\n", __FILE__, __LINE__, #c, g_err.c_str()); \
            g_failed++;                                                 \
        }                                                               \
    } while (0)

struct FakeBackend final : host::DeliveryBackend {
    int wait(void *ev) override
    {
        FakeEvent *e = static_cast<FakeEvent *>(ev);
        const int64_t w = e->want.load(std::memory_order_acquire);
        while (e->done.load(std::memory_order_acquire) < w)
            std::this_thread::yield();
        return SDR_OK;
    }
    int query(void *ev) override
    {
        FakeEvent *e = static_cast<FakeEvent *>(ev);
        return e->done.load(std::memory_order_acquire) >= e->want.load(std::memory_order_acquire) ? SDR_OK : SDR_ERR_WOULD_BLOCK;
    }
    std::unique_ptr<unsigned char[]> copy_used(const unsigned char *block, const host::BatchMeta &) override
    {
        std::unique_ptr<unsigned char[]> p(new unsigned char[BLOCK]);
        memcpy(p.get(), block, BLOCK);
        return p;
    }
    int deliver(const unsigned char *block, const host::BatchMeta &m, void *out) override
    {
        Out *o = static_cast<Out *>(out);
        o->batch = m.batch;
        memcpy(&o->stamp, block, sizeof(int64_t));
        return SDR_OK;
    }
    int report(int code, const char *msg) override
    {
        g_err = msg;
        return code;
    }
};

// slot l of a band is active in batch b unless (b + l) % 3 == 0
bool active(int64_t b, int l) { return (b + l) % 3 != 0; }
sdr_listener_report record(int64_t b, int band, int l)
{
    sdr_listener_report r{};
    r.band = band;
    r.listener = active(b, l) ? l : -1;
    r.bin = 100 * band + l;
    r.ticks = (int32_t)b + 1;
    r.on_sum_q = b * 1000 + band * 10 + l;
    r.wpm = 20.0 + (double)b;
    return r;
}

struct Rig {
    FakeBackend be;
    host::Delivery d{&be, RING, SPAN};
    std::vector<std::unique_ptr<unsigned char[]>> blocks;
    std::vector<std::unique_ptr<sdr_listener_report[]>> reports;
    std::vector<std::unique_ptr<FakeEvent>> ev;
    int64_t next = 0;
    Rig()
    {
        d.grow(RING + SPAN);
        for (int i = 0; i < RING + SPAN; i++) {
            blocks.emplace_back(new unsigned char[BLOCK]());
            reports.emplace_back(new sdr_listener_report[BANDS * STRIDE]);
            memset(reports.back().get(), 0xff, sizeof(sdr_listener_report) * BANDS * STRIDE);  // (as the library allocates it)
            ev.emplace_back(new FakeEvent);
            ev.emplace_back(new FakeEvent);
            d.set(i).block = blocks.back().get();
            d.set(i).reports = reports.back().get();
            d.set(i).ev_listen = ev[2 * (size_t)i].get();
            d.set(i).ev_peaks = ev[2 * (size_t)i + 1].get();
        }
        d.reset(true, 0);
    }
    // the producer's side of one batch (capi_process.hip): park the set's old batch, enqueue, publish
    int enqueue(int slots, bool reports_on, bool complete = true)
    {
        const int64_t b = next++;
        const int si = d.set_index(b);
        CHECK(d.park(si) == SDR_OK);
        host::ResultSet &S = d.set(si);
        static_cast<FakeEvent *>(S.ev_peaks)->want.store(b, std::memory_order_release);
        if (complete)
            static_cast<FakeEvent *>(S.ev_listen)->want.store(b, std::memory_order_release);
        host::BatchMeta m;
        m.batch = b;
        m.frames = 100;
        m.slots = complete ? slots : 0;
        m.reports = complete && reports_on && slots > 0 ? 1 : 0;
        m.report_bands = BANDS;
        m.report_stride = STRIDE;
        d.publish(si, m, complete);
        return si;
    }
    // the device's side: the kernels' writes (the first `slots` slots of every band), then the events
    void finish_listen(int si, int64_t b, int slots, bool reports_on)
    {
        if (reports_on)
            for (int band = 0; band < BANDS; band++)
                for (int l = 0; l < slots; l++)
                    d.set(si).reports[band * STRIDE + l] = record(b, band, l);
        static_cast<FakeEvent *>(d.set(si).ev_listen)->done.store(b, std::memory_order_release);
    }
    void finish_peaks(int si, int64_t b)
    {
        memcpy(d.set(si).block, &b, sizeof b);
        static_cast<FakeEvent *>(d.set(si).ev_peaks)->done.store(b, std::memory_order_release);
    }
    void finish(int si, int64_t b, int slots, bool reports_on)
    {
        finish_listen(si, b, slots, reports_on);
        finish_peaks(si, b);
    }
};

int expected_count(int64_t b, int slots)
{
    int n = 0;
    for (int l = 0; l < slots; l++)
        n += active(b, l) ? BANDS : 0;
    return n;
}

bool reports_are(const sdr_listener_report *got, int64_t b, int slots)
{
    int i = 0;
    for (int band = 0; band < BANDS; band++)
        for (int l = 0; l < slots; l++) {
            if (!active(b, l))
                continue;
            const sdr_listener_report want = record(b, band, l);
            if (memcmp(&got[i++], &want, sizeof want) != 0)
                return false;
        }
    return true;
}

// peek batch `b` (slots listener slots per band; reports on or off), then poll it
void peek_and_poll(Rig &rig, int64_t b, int slots, bool reports_on, bool wait)
{
    sdr_listener_report buf[BANDS * STRIDE];
    host::ReportsOut ro;
    ro.out = buf;
    ro.cap = BANDS * STRIDE;
    CHECK(rig.d.peek_reports(&ro, wait) == SDR_OK);
    const int n = reports_on ? expected_count(b, slots) : 0;
    CHECK(ro.batch == b && ro.n == n);
    CHECK(n == 0 || reports_are(buf, b, slots));
    CHECK(rig.d.deliver_next() == b);  // a peek
    host::ReportsOut again;
    again.out = buf;
    again.cap = BANDS * STRIDE;
    CHECK(rig.d.peek_reports(&again, false) == SDR_OK && again.n == n && again.batch == b);
    Out o;
    CHECK(rig.d.poll(&o, wait) == SDR_OK);
    CHECK(o.batch == b && o.stamp == b);
}

void order()
{
    Rig rig;
    sdr_listener_report buf[BANDS * STRIDE];
    memset(buf, 0, sizeof buf);
    host::ReportsOut ro;
    ro.out = buf;
    ro.cap = BANDS * STRIDE;
    CHECK(rig.d.peek_reports(&ro, false) == SDR_ERR_WOULD_BLOCK);  // nothing processed
    CHECK(rig.d.peek_reports(&ro, true) == SDR_ERR_WOULD_BLOCK);
    const int s0 = rig.enqueue(5, true), s1 = rig.enqueue(4, false), s2 = rig.enqueue(0, true), s3 = rig.enqueue(1, true);
    CHECK(rig.d.peek_reports(&ro, false) == SDR_ERR_WOULD_BLOCK);  // not finished: as poll()
    rig.finish_listen(s0, 0, 5, true);
    CHECK(rig.d.peek_reports(&ro, false) == SDR_ERR_WOULD_BLOCK);  // the spectral half counts too, as for poll()
    Out o;
    CHECK(rig.d.poll(&o, false) == SDR_ERR_WOULD_BLOCK);
    rig.finish_peaks(s0, 0);
    rig.finish(s1, 1, 4, false);
    rig.finish(s2, 2, 0, true);
    rig.finish(s3, 3, 1, true);
    // too small: the count needed, nothing copied, the batch stays; the retry delivers
    const int need = expected_count(0, 5);
    CHECK(need == 6);
    host::ReportsOut small;
    small.out = buf;
    small.cap = need - 1;
    CHECK(rig.d.peek_reports(&small, false) == SDR_ERR_BAD_SIZE && small.n == need && small.batch == 0 && buf[0].ticks == 0);
    small.out = nullptr;
    small.cap = 0;
    CHECK(rig.d.peek_reports(&small, true) == SDR_ERR_BAD_SIZE && small.n == need);
    CHECK(rig.d.deliver_next() == 0);
    peek_and_poll(rig, 0, 5, true, false);
    peek_and_poll(rig, 1, 4, false, false);  // processed with reports off
    peek_and_poll(rig, 2, 0, true, true);    // no listener slot
    peek_and_poll(rig, 3, 1, true, true);    // batch 3, slot 0: (3 + 0) % 3 == 0 - the only slot is not active
    CHECK(expected_count(3, 1) == 0);
    CHECK(rig.d.peek_reports(&ro, true) == SDR_ERR_WOULD_BLOCK);
}

void park()
{
    Rig rig;
    for (int b = 0; b < 10; b++) {
        if (b >= RING)
            CHECK(rig.d.parked_count() == (size_t)(b - RING));
        const int si = rig.enqueue(1 + b % STRIDE, b != 2);  // (batch 2: reports off)
        rig.finish(si, b, 1 + b % STRIDE, b != 2);
    }
    CHECK(rig.d.parked_count() == 4);
    for (int b = 0; b < 10; b++)
        peek_and_poll(rig, b, 1 + b % STRIDE, b != 2, b % 2 == 0);
    CHECK(rig.d.parked_count() == 0 && rig.d.pending() == 0);
}

void deferred()
{
    Rig rig;
    const int si = rig.enqueue(0, true, false);  // the spectral half only: no listener is bound yet
    sdr_listener_report buf[BANDS * STRIDE];
    host::ReportsOut ro;
    ro.out = buf;
    ro.cap = BANDS * STRIDE;
    rig.finish_peaks(si, 0);
    CHECK(rig.d.peek_reports(&ro, false) == SDR_ERR_WOULD_BLOCK);  // the reports belong to the listen half
    CHECK(rig.d.peek_reports(&ro, true) == SDR_ERR_WOULD_BLOCK);
    Out o;
    CHECK(rig.d.poll(&o, false) == SDR_ERR_WOULD_BLOCK);
    static_cast<FakeEvent *>(rig.d.set(si).ev_listen)->want.store(0, std::memory_order_release);
    rig.d.complete(si, 4, 0, 1);  // the listen half is enqueued: four slots by now, reports on
    CHECK(rig.d.peek_reports(&ro, false) == SDR_ERR_WOULD_BLOCK);  // whole now, not finished
    rig.finish_listen(si, 0, 4, true);
    peek_and_poll(rig, 0, 4, true, false);
    // ... and one whose listen half ran with reports off: complete() says so
    const int s1 = rig.enqueue(0, true, false);
    rig.finish_peaks(s1, 1);
    static_cast<FakeEvent *>(rig.d.set(s1).ev_listen)->want.store(1, std::memory_order_release);
    rig.d.complete(s1, 4, 1, 0);
    rig.finish_listen(s1, 1, 4, false);
    peek_and_poll(rig, 1, 4, false, true);
}

void graph()
{
    Rig rig;
    for (int b = 0; b < 2; b++)
        rig.finish(rig.enqueue(3, true), b, 3, true);
    // (sdr_graph_capture parks the eager ring's sets first)
    for (int i = 0; i < RING; i++)
        CHECK(rig.d.park(i) == SDR_OK);
    rig.d.graph_begin(rig.next);
    for (int b = 2; b < 2 + SPAN + 3; b++)  // more than the graph sets hold: the oldest are parked on reuse
        rig.finish(rig.enqueue(5, true), b, 5, true);
    CHECK(rig.d.graph_end(rig.next) == SDR_OK);
    CHECK(rig.d.parked_count() == (size_t)rig.next);
    const int64_t graph_batches = rig.next;
    for (int b = 0; b < 3; b++)  // eager again
        rig.finish(rig.enqueue(2, true), graph_batches + b, 2, true);
    for (int64_t b = 0; b < rig.next; b++)
        peek_and_poll(rig, b, b < 2 ? 3 : b < graph_batches ? 5 : 2, true, b % 3 == 0);
}

}  // namespace

int main()
{
    struct {
        const char *name;
        void (*run)();
    } const tests[] = {{"order", order}, {"park", park}, {"deferred", deferred}, {"graph", graph}};
    for (const auto &t : tests) {
        const int before = g_failed;
        t.run();
        printf("%s %s\n", t.name, g_failed == before ? "ok" : "FAILED");
    }
    return g_failed ? 1 : 0;
}
