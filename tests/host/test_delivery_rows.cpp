// Host-only model test of bulk delivery with a row block (sdrainer_amd/csrc/host/delivery.h - the code the library runs
// behind sdr_poll_rows, not a copy): fake events, a block and a row block per set, stamped with the batch the way the pack
// kernels and k_cum_rows fill them.  Checked: peek_rows looks at the batch the next poll() hands out and leaves it
// undelivered; it blocks exactly where poll() would (and, for a batch whose listen half is still to come, only on the
// spectral half's event); a buffer too small is refused with the count needed and the retry delivers; a batch parked on
// the host - ring reuse, the end of graph mode - takes its rows with it, and rows and batches arrive oldest first; a batch
// without rows delivers none.  Built with the sanitizers by tests/test_delivery_rows.py.  No GPU, no HIP.
//
// Scenarios:
//   order      publish, peek (not finished / finished), BAD_SIZE and retry, poll, a batch with rows off, one without chunks
//   park       ten batches, nobody polls: the first four are parked with their rows when their sets are reused
//   deferred   a batch published without its listen half: rows as soon as the spectral half is done, the batch only later
//   graph      graph sets, then graph_end: what was not polled is parked with its rows; eager batches follow
//   threads    a producer that runs ahead of a consumer thread which peeks, then polls, each batch (ThreadSanitizer)
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../sdrainer_amd/csrc/host/delivery.h"

namespace {

constexpr int RING = 6, SPAN = 12, COLUMNS = 8, MAX_ROWS = 4;
constexpr size_t BLOCK = 16;

struct FakeEvent {
    std::atomic<int64_t> done{-1}, want{-1};
};

struct Out {
    int64_t batch = -1, stamp = -1;
};

thread_local std::string g_err;
std::atomic<int> g_failed{0};
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

float row_value(int64_t batch, int row, int col) { return (float)(batch * 1000 + row * 10 + col); }

struct Rig {
    FakeBackend be;
    host::Delivery d{&be, RING, SPAN};
    std::vector<std::unique_ptr<unsigned char[]>> blocks;
    std::vector<std::unique_ptr<float[]>> rows;
    std::vector<std::unique_ptr<FakeEvent>> ev;
    int64_t next = 0;
    Rig()
    {
        d.grow(RING + SPAN);
        for (int i = 0; i < RING + SPAN; i++) {
            blocks.emplace_back(new unsigned char[BLOCK]());
            rows.emplace_back(new float[MAX_ROWS * COLUMNS]());
            ev.emplace_back(new FakeEvent);
            ev.emplace_back(new FakeEvent);
            d.set(i).block = blocks.back().get();
            d.set(i).rows = rows.back().get();
            d.set(i).ev_listen = ev[2 * (size_t)i].get();
            d.set(i).ev_peaks = ev[2 * (size_t)i + 1].get();
        }
        d.reset(true, 0);
    }
    // the producer's side of one batch (capi_process.hip): park the set's old batch, enqueue, publish
    int enqueue(int n_rows, int columns, bool complete = true)
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
        m.chunks = n_rows;
        m.rows = columns ? n_rows : 0;
        m.row_columns = columns;
        d.publish(si, m, complete);
        return si;
    }
    // the device's side: the kernels' writes, then the events
    void finish_peaks(int si, int64_t b, int n_rows)
    {
        memcpy(d.set(si).block, &b, sizeof b);
        for (int r = 0; r < n_rows; r++)
            for (int c = 0; c < COLUMNS; c++)
                d.set(si).rows[r * COLUMNS + c] = row_value(b, r, c);
        static_cast<FakeEvent *>(d.set(si).ev_peaks)->done.store(b, std::memory_order_release);
    }
    void finish_listen(int si, int64_t b) { static_cast<FakeEvent *>(d.set(si).ev_listen)->done.store(b, std::memory_order_release); }
    void finish(int si, int64_t b, int n_rows)
    {
        finish_peaks(si, b, n_rows);
        finish_listen(si, b);
    }
};

bool rows_are(const float *rows, int64_t batch, int n_rows)
{
    for (int r = 0; r < n_rows; r++)
        for (int c = 0; c < COLUMNS; c++)
            if (rows[r * COLUMNS + c] != row_value(batch, r, c))
                return false;
    return true;
}

// peek batch `b` with `n_rows` rows, then poll it
void peek_and_poll(Rig &rig, int64_t b, int n_rows, bool wait)
{
    float buf[MAX_ROWS * COLUMNS];
    host::RowsOut ro;
    ro.rows = buf;
    ro.rows_cap = MAX_ROWS;
    CHECK(rig.d.peek_rows(&ro, wait) == SDR_OK);
    CHECK(ro.batch == b && ro.n_rows == n_rows && (n_rows == 0 || ro.columns == COLUMNS));
    CHECK(rows_are(buf, b, ro.n_rows));
    CHECK(rig.d.deliver_next() == b);  // a peek
    Out o;
    CHECK(rig.d.poll(&o, wait) == SDR_OK);
    CHECK(o.batch == b && o.stamp == b);
}

void order()
{
    Rig rig;
    float buf[MAX_ROWS * COLUMNS] = {};
    host::RowsOut ro;
    ro.rows = buf;
    ro.rows_cap = MAX_ROWS;
    CHECK(rig.d.peek_rows(&ro, false) == SDR_ERR_WOULD_BLOCK);  // nothing processed
    const int s0 = rig.enqueue(3, COLUMNS), s1 = rig.enqueue(2, 0), s2 = rig.enqueue(0, COLUMNS), s3 = rig.enqueue(1, COLUMNS);
    CHECK(rig.d.peek_rows(&ro, false) == SDR_ERR_WOULD_BLOCK);  // not finished: as poll()
    Out o;
    CHECK(rig.d.poll(&o, false) == SDR_ERR_WOULD_BLOCK);
    rig.finish_peaks(s0, 0, 3);
    CHECK(rig.d.peek_rows(&ro, false) == SDR_ERR_WOULD_BLOCK);  // a whole batch: its listen half counts, as for poll()
    rig.finish_listen(s0, 0);
    rig.finish(s1, 1, 0);
    rig.finish(s2, 2, 0);
    rig.finish(s3, 3, 1);
    // too small: the count needed, nothing copied, the batch stays; the retry delivers
    host::RowsOut small;
    small.rows = buf;
    small.rows_cap = 2;
    CHECK(rig.d.peek_rows(&small, false) == SDR_ERR_BAD_SIZE && small.n_rows == 3 && small.batch == 0 && buf[0] == 0.f);
    small.rows = nullptr;
    small.rows_cap = 0;
    CHECK(rig.d.peek_rows(&small, true) == SDR_ERR_BAD_SIZE && small.n_rows == 3);
    peek_and_poll(rig, 0, 3, false);
    peek_and_poll(rig, 1, 0, false);  // processed with rows off
    peek_and_poll(rig, 2, 0, true);   // completed no cumulation
    peek_and_poll(rig, 3, 1, true);
    CHECK(rig.d.peek_rows(&ro, true) == SDR_ERR_WOULD_BLOCK);
}

void park()
{
    Rig rig;
    std::vector<int> n_rows;
    for (int b = 0; b < 10; b++) {
        if (b >= RING)
            CHECK(rig.d.parked_count() == (size_t)(b - RING));
        n_rows.push_back(1 + b % MAX_ROWS);
        const int si = rig.enqueue(n_rows.back(), b == 2 ? 0 : COLUMNS);  // (batch 2: rows off)
        rig.finish(si, b, b == 2 ? 0 : n_rows.back());
    }
    CHECK(rig.d.parked_count() == 4);
    for (int b = 0; b < 10; b++)
        peek_and_poll(rig, b, b == 2 ? 0 : n_rows[(size_t)b], b % 2 == 0);
    CHECK(rig.d.parked_count() == 0 && rig.d.pending() == 0);
}

void deferred()
{
    Rig rig;
    const int si = rig.enqueue(2, COLUMNS, false);  // the spectral half only
    float buf[MAX_ROWS * COLUMNS];
    host::RowsOut ro;
    ro.rows = buf;
    ro.rows_cap = MAX_ROWS;
    CHECK(rig.d.peek_rows(&ro, false) == SDR_ERR_WOULD_BLOCK);
    rig.finish_peaks(si, 0, 2);
    CHECK(rig.d.peek_rows(&ro, false) == SDR_OK && ro.batch == 0 && ro.n_rows == 2 && rows_are(buf, 0, 2));
    CHECK(rig.d.peek_rows(&ro, true) == SDR_OK && ro.n_rows == 2);
    Out o;
    CHECK(rig.d.poll(&o, false) == SDR_ERR_WOULD_BLOCK);  // the batch itself waits for its listen half
    static_cast<FakeEvent *>(rig.d.set(si).ev_listen)->want.store(0, std::memory_order_release);
    rig.d.complete(si, 5, 0);
    CHECK(rig.d.peek_rows(&ro, false) == SDR_ERR_WOULD_BLOCK);  // whole now: as poll()
    rig.finish_listen(si, 0);
    peek_and_poll(rig, 0, 2, false);
}

void graph()
{
    Rig rig;
    for (int b = 0; b < 2; b++)
        rig.finish(rig.enqueue(1, COLUMNS), b, 1);
    // (sdr_graph_capture parks the eager ring's sets first)
    for (int i = 0; i < RING; i++)
        CHECK(rig.d.park(i) == SDR_OK);
    rig.d.graph_begin(rig.next);
    for (int b = 2; b < 2 + SPAN + 3; b++)  // more than the graph sets hold: the oldest are parked on reuse
        rig.finish(rig.enqueue(2, COLUMNS), b, 2);
    CHECK(rig.d.graph_end(rig.next) == SDR_OK);
    CHECK(rig.d.parked_count() == (size_t)rig.next);
    const int64_t graph_batches = rig.next;
    for (int b = 0; b < 3; b++)  // eager again
        rig.finish(rig.enqueue(3, COLUMNS), graph_batches + b, 3);
    for (int64_t b = 0; b < rig.next; b++)
        peek_and_poll(rig, b, b < 2 ? 1 : b < graph_batches ? 2 : 3, b % 3 == 0);
}

void threads()
{
    Rig rig;
    constexpr int N = 400;
    int seen = 0;
    std::thread consumer([&] {
        float buf[MAX_ROWS * COLUMNS];
        while (seen < N) {
            host::RowsOut ro;
            ro.rows = buf;
            ro.rows_cap = MAX_ROWS;
            const int rc = rig.d.peek_rows(&ro, true);
            if (rc == SDR_ERR_WOULD_BLOCK) {
                std::this_thread::yield();
                continue;
            }
            CHECK(rc == SDR_OK && ro.batch == seen && ro.n_rows == 1 + seen % MAX_ROWS && rows_are(buf, ro.batch, ro.n_rows));
            Out o;
            int prc;
            while ((prc = rig.d.poll(&o, true)) == SDR_ERR_WOULD_BLOCK)
                std::this_thread::yield();
            CHECK(prc == SDR_OK && o.batch == seen && o.stamp == seen);
            seen++;
        }
    });
    for (int b = 0; b < N; b++) {
        const int n = 1 + b % MAX_ROWS;
        // (the producer is its own device here: park() waits for the set's events, so they complete before the next reuse)
        const int si = rig.enqueue(n, COLUMNS);
        rig.finish(si, b, n);
        if (b % 7 == 0)
            std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    consumer.join();
    CHECK(seen == N && rig.d.pending() == 0);
}

}  // namespace

int main()
{
    struct {
        const char *name;
        void (*run)();
    } const tests[] = {{"order", order}, {"park", park}, {"deferred", deferred}, {"graph", graph}, {"threads", threads}};
    for (const auto &t : tests) {
        const int before = g_failed;
        t.run();
        printf("%s %s\n", t.name, g_failed == before ? "ok" : "FAILED");
    }
    return g_failed ? 1 : 0;
}
