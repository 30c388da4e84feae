// host/staging.h without a GPU: the kind table, and the row arithmetic of the staged host input against a model that
// moves real bytes.  Five bands, one of each kind (float32, KiwiSDR int16, sc16, cs8, cu8), each with a pseudo-random
// stream; three staging sets whose pinned and device buffers are plain byte vectors of exactly the bank's sizes.  Pushes
// come in pieces of 1, 3 and 7 hops until StreamStage::would_drop refuses, batches are taken whole or cut by a limit, and
// every copy sdr_process_staged_limit issues (capi_staged.hip) is a memcpy of the planned range: the upload, a trivial
// unpack (each raw value widened to the four bytes a float32 takes), the history copy, the leftover move.  After every
// batch the samples [0, span) of each band's float32 device row must be the band's stream at the frames the batch covers.
// A planned range outside its buffer fails a check (and is fatal under -fsanitize=address).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../sdrainer_amd/csrc/host/staging.h"

using sdr::StagedKind;

static int failures = 0;
#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);          \
            failures++;                                                       \
        }                                                                     \
    } while (0)

static const StagedKind kKinds[] = {StagedKind::F32, StagedKind::Be16, StagedKind::Sc16, StagedKind::Cs8, StagedKind::Cu8};
constexpr int kBands = 5, kRing = 3;

static void test_kind_table()
{
    // float32: a row sample is 8 bytes and there is no raw buffer
    const sdr::StagedKindInfo f = sdr::staged_kind_info(StagedKind::F32);
    CHECK(f.value_bytes == 4 && f.row_sample_bytes == 8 && !f.raw);
    // int16, big-endian or not: a row sample is 4 bytes, a value 2
    for (StagedKind k : {StagedKind::Be16, StagedKind::Sc16}) {
        const sdr::StagedKindInfo i = sdr::staged_kind_info(k);
        CHECK(i.value_bytes == 2 && i.row_sample_bytes == 4 && i.raw);
        CHECK(sdr::staged_sample_bytes(k) == i.row_sample_bytes);
    }
    // 8-bit: a row sample is 4 bytes, a value 1: a band fills half its row
    for (StagedKind k : {StagedKind::Cs8, StagedKind::Cu8}) {
        const sdr::StagedKindInfo i = sdr::staged_kind_info(k);
        CHECK(i.value_bytes == 1 && i.row_sample_bytes == 4 && i.raw);
        CHECK(2 * sdr::staged_sample_bytes(k) == i.row_sample_bytes);
    }
    CHECK(!sdr::staged_kind_info(StagedKind::None).raw && sdr::staged_kind_info(StagedKind::None).value_bytes == 0);
    // the refusals, byte for byte what sdr_push_iq, sdr_push_kiwi_snd, sdr_push_iq_sc16 and sdr_push_iq8 (cs8, cu8) say
    CHECK(!strcmp(f.mixed, "band already holds int16 (KiwiSDR or sc16) or 8-bit frames in this batch"));
    CHECK(!strcmp(sdr::staged_kind_info(StagedKind::Be16).mixed, "band already holds float32, sc16 or 8-bit frames in this batch"));
    CHECK(!strcmp(sdr::staged_kind_info(StagedKind::Sc16).mixed, "band already holds float32, KiwiSDR or 8-bit frames in this batch"));
    CHECK(!strcmp(sdr::staged_kind_info(StagedKind::Cs8).mixed, "band already holds float32, int16 or cu8 frames in this batch"));
    CHECK(!strcmp(sdr::staged_kind_info(StagedKind::Cu8).mixed, "band already holds float32, int16 or cs8 frames in this batch"));
    // a set's buffers: float32 rows of 8 bytes per sample, raw rows of 4
    CHECK(sdr::staging_buffer_bytes(false, 1000, 3) == 24000 && sdr::staging_buffer_bytes(true, 1000, 3) == 12000);
    printf("kinds ok\n");
}

// dst[off, off + bytes) <- src[from, from + bytes), both ranges inside their buffers
static void copy_checked(std::vector<uint8_t> &dst, size_t off, const std::vector<uint8_t> &src, size_t from, size_t bytes)
{
    const bool inside = off <= dst.size() && bytes <= dst.size() - off && from <= src.size() && bytes <= src.size() - from;
    CHECK(inside);
    if (inside && bytes)
        memcpy(dst.data() + off, src.data() + from, bytes);
}

// The model's unpack kernel: value i of `n` raw values of `vb` bytes each becomes the four bytes at dst + 4 * i (the value,
// zero-extended) - one float32 per value, as k_unpack.hip writes.  vb = 4: float32 values as they are.
template <size_t VB>
static void widen_values(uint8_t *dst, const uint8_t *src, size_t n)
{
    for (size_t i = 0; i < n; i++) {
        uint32_t v = 0;
        memcpy(&v, src + i * VB, VB);
        memcpy(dst + 4 * i, &v, 4);
    }
}
static void widen(uint8_t *dst, const uint8_t *src, size_t vb, size_t n)
{
    if (vb == 1)
        widen_values<1>(dst, src, n);
    else if (vb == 2)
        widen_values<2>(dst, src, n);
    else
        memcpy(dst, src, 4 * n);
}

struct Set {
    std::vector<uint8_t> h_f32, h_raw, d_f32, d_raw;
};

struct Band {
    StagedKind kind;
    size_t vb;                    // bytes per value
    std::vector<uint8_t> stream;  // the whole stream, 2 values per sample
    sdr::StreamStage ss;
    size_t pushed = 0;  // samples
    int streak = 0, best_streak = 0;  // consecutive batches that left samples staged
};

static int longest_streak[kBands];

static void run(int n, int hop, int piece_hops, int limit, int max_batch)
{
    const size_t cap = sdr::span_samples(max_batch, hop, n);
    const size_t total_hops = (size_t)max_batch + 5 * (size_t)std::min(limit, max_batch) + (size_t)(n / hop);
    const size_t total = total_hops * (size_t)hop;  // samples per band
    uint64_t x = 0x9e3779b97f4a7c15ull ^ ((uint64_t)n << 32) ^ ((uint64_t)hop << 8) ^ (uint64_t)(piece_hops * 131 + limit * 7 + max_batch);
    std::vector<Band> bands((size_t)kBands);
    for (int b = 0; b < kBands; b++) {
        Band &B = bands[(size_t)b];
        B.kind = kKinds[b];
        B.vb = sdr::staged_kind_info(B.kind).value_bytes;
        B.ss = sdr::StreamStage{n, hop, 0, 0};
        B.stream.resize(((2 * total * B.vb) + 7) & ~(size_t)7);
        for (size_t i = 0; i < B.stream.size(); i += 8) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            memcpy(B.stream.data() + i, &x, 8);
        }
    }
    Set sets[kRing];
    for (Set &s : sets) {  // (stale bytes everywhere: nothing may be right by accident)
        s.h_f32.assign(sdr::staging_buffer_bytes(false, cap, kBands), 0xa5);
        s.d_f32.assign(sdr::staging_buffer_bytes(false, cap, kBands), 0x5a);
        s.h_raw.assign(sdr::staging_buffer_bytes(true, cap, kBands), 0xc3);
        s.d_raw.assign(sdr::staging_buffer_bytes(true, cap, kBands), 0x3c);
    }
    std::vector<uint8_t> want_row;
    int cur = 0, batches = 0, round = 0;
    size_t consumed = 0;  // frames
    for (;; round++) {
        // pushes (sdr_push_*: push_samples), each band until its set is full; one band in three sits a round out
        for (int b = 0; b < kBands; b++) {
            Band &B = bands[(size_t)b];
            if ((round + b) % 3 == 0)
                continue;
            while (B.pushed < total) {
                const size_t ns = std::min((size_t)piece_hops * (size_t)hop, total - B.pushed);
                if (B.ss.would_drop(ns, max_batch))
                    break;
                const sdr::StagedPush at = sdr::staged_push(B.kind, b, cap, B.ss.staged, 2 * ns);
                CHECK(at.bytes == 2 * ns * B.vb);
                Set &S = sets[cur];
                copy_checked(sdr::staged_kind_info(B.kind).raw ? S.h_raw : S.h_f32, at.offset, B.stream, 2 * B.pushed * B.vb, at.bytes);
                B.ss.push(ns);
                B.pushed += ns;
            }
        }
        // the batch (sdr_process_staged_limit)
        int take = std::min(max_batch, limit);
        bool all_pushed = true;
        for (const Band &B : bands) {
            take = std::min(take, B.ss.frames());
            all_pushed = all_pushed && B.pushed == total;
        }
        if (take == 0) {
            if (all_pushed)
                break;
            continue;
        }
        const size_t span = sdr::span_samples(take, hop, n);
        const int next = (cur + 1) % kRing;
        Set &S = sets[cur], &NX = sets[next];
        for (int b = 0; b < kBands; b++) {
            const Band &B = bands[(size_t)b];
            const sdr::StagedUpload up = sdr::staged_upload(B.kind, b, cap, B.ss.history, span);
            CHECK(up.n_values == 2 * (span - B.ss.history));
            if (sdr::staged_kind_info(B.kind).raw) {
                copy_checked(S.d_raw, up.raw_offset, S.h_raw, up.src_offset, up.bytes);
                // the unpack kernel: n_values raw values from raw_offset, one float32 each from sample f32_sample on
                const size_t dst = up.f32_sample * 8;
                const bool inside = dst <= S.d_f32.size() && up.n_values * 4 <= S.d_f32.size() - dst && up.raw_offset <= S.d_raw.size() &&
                                    up.n_values * B.vb <= S.d_raw.size() - up.raw_offset;
                CHECK(inside);
                CHECK(up.n_values * B.vb == up.bytes);
                if (inside)
                    widen(S.d_f32.data() + dst, S.d_raw.data() + up.raw_offset, B.vb, up.n_values);
            } else {
                copy_checked(S.d_f32, up.f32_sample * 8, S.h_f32, up.src_offset, up.bytes);
            }
        }
        // what the FFT reads: samples [0, span) of every band's row are the stream from frame `consumed` on
        for (int b = 0; b < kBands; b++) {
            const Band &B = bands[(size_t)b];
            const uint8_t *row = S.d_f32.data() + (size_t)b * cap * 8;
            want_row.resize(8 * span);
            widen(want_row.data(), B.stream.data() + 2 * consumed * (size_t)hop * B.vb, B.vb, 2 * span);
            if (memcmp(row, want_row.data(), 8 * span) != 0) {
                printf("FAILED n %d hop %d piece %d limit %d max_batch %d: band %d batch %d (frames %zu..%zu) reads other samples\n", n, hop, piece_hops,
                       limit, max_batch, b, batches, consumed, consumed + (size_t)take);
                failures++;
            }
        }
        if (n > hop) {  // the next batch's history, row by row as the one 2D copy moves it
            const sdr::StagedHistory h = sdr::staged_history(cap, (size_t)take * (size_t)hop, (size_t)(n - hop));
            CHECK(h.pitch * kBands == S.d_f32.size() && h.src_offset + h.width <= h.pitch);
            for (int b = 0; b < kBands; b++)
                copy_checked(NX.d_f32, (size_t)b * h.pitch, S.d_f32, h.src_offset + (size_t)b * h.pitch, h.width);
        }
        for (int b = 0; b < kBands; b++) {
            Band &B = bands[(size_t)b];
            const sdr::StreamStage::Consumed t = B.ss.consume(take);
            if (t.left > 0) {
                const sdr::StagedLeft mv = sdr::staged_left(B.kind, b, cap, t);
                const bool raw = sdr::staged_kind_info(B.kind).raw;
                copy_checked(raw ? NX.h_raw : NX.h_f32, mv.dst_offset, raw ? S.h_raw : S.h_f32, mv.src_offset, mv.bytes);
                B.streak++;
            } else {
                B.streak = 0;
            }
            B.best_streak = std::max(B.best_streak, B.streak);
        }
        consumed += (size_t)take;
        cur = next;
        batches++;
    }
    CHECK(consumed == total_hops - (size_t)(n / hop - 1));  // every complete frame of the stream, once
    CHECK(batches >= 5);                                    // every set used, the first one twice
    for (int b = 0; b < kBands; b++) {
        // one frame at a time out of a set that pushes of any piece size fill with six or more: a band's leftovers go
        // round the three-set ring more than once
        if (limit == 1)
            CHECK(bands[(size_t)b].best_streak >= 4);
        longest_streak[b] = std::max(longest_streak[b], bands[(size_t)b].best_streak);
    }
}

int main()
{
    test_kind_table();
    for (int max_batch : {8, 64})
        for (int piece : {1, 3, 7})
            for (int limit : {1000000, 5, 1}) {
                for (int hop : {512, 256, 32})
                    run(512, hop, piece, limit, max_batch);
                for (int hop : {16384, 1024})
                    run(16384, hop, piece, limit, max_batch);
            }
    for (int b = 0; b < kBands; b++)
        CHECK(longest_streak[b] >= 4);
    printf("rows ok\n");
    return failures ? 1 : 0;
}
