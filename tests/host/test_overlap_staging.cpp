// host/overlap.h without a GPU: which hops sdr_create takes, the input index function of the FFT kernels, and the
// arithmetic of the staged host input (sdr_push_iq on a bank with hop <= block_size) against a model that counts
// absolute sample positions: a stream pushed in pieces of 1, 3 and 7 hops, batches cut by a limit
// (sdr_process_staged_limit) or taken whole, at hop = N, N / 2 and N / 16.
#include <algorithm>
#include <cstdio>

#include "../../sdrainer_amd/csrc/host/overlap.h"

static int failures = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            failures++;                                                       \
        }                                                                     \
    } while (0)

static void test_hops()
{
    for (int n = 512; n <= 65536; n *= 2) {
        CHECK(sdr::hop_valid(0, n) && sdr::effective_hop(0, n) == n);
        for (int hop = -4; hop <= 2 * n; hop++) {
            const bool pow2 = hop > 0 && (hop & (hop - 1)) == 0;
            const bool want = hop == 0 || (pow2 && hop >= 32 && hop * 16 >= n && hop <= n);
            if (sdr::hop_valid(hop, n) != want) {
                printf("FAILED hop_valid(%d, %d)\n", hop, n);
                failures++;
            }
        }
        CHECK(sdr::effective_hop(n / 4, n) == n / 4);
    }
    printf("hops ok\n");
}

static void test_index()
{
    // band b, frame f -> b * band_stride + f * frame_stride; dense frames are frame_stride = N, band_stride = frames * N
    CHECK(sdr::input_sample_offset(0, 0, 4096) == 0);
    CHECK(sdr::input_sample_offset(3 * (size_t)1000, 7, 128) == 3000 + 7 * 128);
    const size_t n = 65536, frames = 8192;
    CHECK(sdr::input_sample_offset(7 * frames * n, 8191, (int)n) == 7 * frames * n + 8191 * n);  // (beyond 32 bits)
    CHECK(sdr::span_samples(0, 128, 512) == 0 && sdr::span_samples(1, 128, 512) == 512 && sdr::span_samples(300, 128, 512) == 299 * 128 + 512);
    // the last sample a batch reads lies inside what the caller guarantees
    for (int hop : {32, 512, 4096})
        for (int k : {1, 2, 100})
            CHECK(sdr::input_sample_offset(0, (unsigned)(k - 1), hop) + 4096 == sdr::span_samples(k, hop, 4096));
    printf("index ok\n");
}

// the stream in absolute samples: `pushed` so far, frames consumed so far, samples on the device up to `device_end`
struct Model {
    long long n, hop, pushed = 0, consumed = 0, device_end = 0;
    long long frames() const
    {
        long long f = 0;  // frames f >= consumed whose last sample has been pushed
        while ((consumed + f) * hop + n <= pushed)
            f++;
        return f;
    }
};

static void run(int n, int hop, int piece_hops, int limit, int max_batch)
{
    sdr::StreamStage st{n, hop, 0, 0};
    Model m{n, hop};
    const long long total_hops = 400;
    long long pushed_hops = 0;
    int batches = 0;
    while (pushed_hops < total_hops || m.frames() > 0) {
        const long long k = std::min<long long>(piece_hops, total_hops - pushed_hops);
        if (k > 0) {
            if (st.would_drop((size_t)(k * hop), max_batch)) {
                // the staging set holds (max_batch - 1) * hop + n samples, history included
                CHECK(st.history + st.staged + (size_t)(k * hop) > (size_t)((max_batch - 1) * (long long)hop + n));
            } else {
                st.push((size_t)(k * hop));
                m.pushed += k * hop;
                pushed_hops += k;
            }
        }
        CHECK(st.frames() == (int)m.frames());
        CHECK(st.history == (size_t)(m.device_end - m.consumed * hop));
        CHECK(st.history + st.staged == (size_t)(m.pushed - m.consumed * hop));
        CHECK(st.history + st.staged <= st.capacity(max_batch));
        const int take = std::min(std::min(st.frames(), limit), max_batch);
        if (take == 0)
            continue;
        const size_t staged_before = st.staged;
        const sdr::StreamStage::Consumed c = st.consume(take);
        const long long span_end = (m.consumed + take - 1) * hop + n;  // one past the last sample the batch reads
        CHECK((long long)c.uploaded == span_end - m.device_end);       // only what is not on the device yet goes up
        CHECK(c.left == staged_before - c.uploaded && c.left_from == c.uploaded);
        CHECK((long long)c.keep_from == (long long)take * hop);        // the history: from the next frame's first sample ...
        CHECK(st.history == (size_t)(n - hop));                        // ... to the end of what the batch read
        CHECK(c.keep_from + st.history == (size_t)(span_end - m.consumed * hop));
        m.device_end = span_end;
        m.consumed += take;
        CHECK(st.staged == (size_t)(m.pushed - m.device_end));
        batches++;
    }
    CHECK(m.consumed == total_hops - (n / hop - 1));  // every complete frame of the stream, once
    CHECK(batches > 0);
}

int main()
{
    test_hops();
    test_index();
    for (int n : {512, 16384})
        for (int hop : {n, n / 2, n / 16})
            for (int piece : {1, 3, 7})
                for (int limit : {1000000, 5, 1}) {
                    run(n, hop, piece, limit, 64);
                    run(n, hop, piece, limit, 8);
                }
    printf("staging ok\n");
    return failures ? 1 : 0;
}
