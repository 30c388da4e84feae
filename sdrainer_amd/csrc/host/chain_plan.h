// chain_plan.h — the plan of the receive chain (include/sdrainer_hip.h "receive chain"): which samples a push uploads, which
// pieces it processes and where their outputs land in the ring, when the ring's carry moves and which bank batches follow.
// Pure integer C++ without HIP: capi_chain.hip executes the actions, tests/host/test_chain_plan.cpp prints them for random
// geometries and tests/chain_ref.py restates them in Python.  All quantities are samples: WIDE samples for the raw buffer and
// the pieces, NARROW samples per band for the ring.
#pragma once
#include <cstdint>
#include <vector>

namespace sdr {

inline int64_t chain_gcd(int64_t a, int64_t b)
{
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}
inline int64_t chain_lcm(int64_t a, int64_t b) { return a / chain_gcd(a, b) * b; }

// G = lcm(2 * Dtot, nb block, 16): the 2 keeps every stage's float32 I,Q output pointer 16-byte aligned (m = p / Dtot is
// even), the 16 keeps a piece's start aligned for one-byte real formats.  nb_block = 1 without a blanker.  -1: an argument
// below 1 (or so large that G would leave 2^62).
inline int64_t chain_granule(int64_t total_decimation, int64_t nb_block)
{
    if (total_decimation < 1 || nb_block < 1 || total_decimation > (int64_t(1) << 40) || nb_block > (int64_t(1) << 16))
        return -1;
    return chain_lcm(chain_lcm(2 * total_decimation, nb_block), 16);
}

// the largest multiple of G within `limit`, the smallest of the members' max_in_samples in wide samples (the fine
// converter's counted times stage one's decimation); 0: not even one granule fits; -1: an argument below 1
inline int64_t chain_piece(int64_t granule, int64_t limit)
{
    if (granule < 1 || limit < 1)
        return -1;
    return limit / granule * granule;
}

// 2 * block_size + piece / Dtot, rounded up to 4: a piece always fits behind fewer than block_size unconsumed samples, and
// the carry's move never overlaps (it happens only with more than 2 * block_size samples resident, of which fewer than
// block_size move).  -1: an argument below 1, hop above block_size, or a piece that is no multiple of Dtot.
inline int64_t chain_min_ring(int64_t block_size, int64_t hop, int64_t piece, int64_t total_decimation)
{
    if (block_size < 1 || hop < 1 || hop > block_size || piece < 1 || total_decimation < 1 || piece % total_decimation != 0)
        return -1;
    if (block_size > (int64_t(1) << 40) || piece > (int64_t(1) << 60))
        return -1;
    return (2 * block_size + piece / total_decimation + 3) / 4 * 4;
}

struct ChainGeometry {
    int64_t total_decimation;  // Dtot
    int64_t granule;           // G
    int64_t piece;             // wide samples per piece at the most, a multiple of G
    int64_t ring;              // narrow samples per band the ring holds, >= chain_min_ring
    int64_t block_size, hop;   // the bank's (hop the effective one)
    int64_t max_batch_frames;  // the bank's
    int64_t max_in;            // wide samples per push at the most
};

enum class ChainOp { Upload, Piece, Move, Batch, Keep };

// Upload  a: the raw buffer's sample the push's first sample goes to (= pending), b: samples
// Piece   a: input offset of the piece (from the raw buffer's front, or from the caller's pointer), b: wide samples p,
//         c: ring offset its p / Dtot narrow samples per band go to
// Move    a: ring offset of the unconsumed samples, b: where they go (0), c: how many per band (may be 0: nothing is copied)
// Batch   a: ring offset of the first frame, b: frames
// Keep    a: raw-buffer offset of the samples left pending, b: where they go (0), c: how many
struct ChainAction {
    ChainOp op;
    int64_t a, b, c;
};

struct ChainPlan {
    ChainGeometry g{};
    int64_t accepted = 0, processed = 0, pending = 0;  // wide samples
    int64_t base = 0, have = 0;                        // the ring holds narrow samples [base, have)
    int64_t frames = 0, batches = 0, moves = 0;

    enum Refusal { Ok = 0, BadSize, State };
    Refusal check(int64_t n, bool host) const
    {
        if (n < 1 || n > g.max_in)
            return BadSize;
        if (!host && n % g.granule != 0)
            return BadSize;
        if (!host && pending != 0)
            return State;
        return Ok;
    }

    // an accepted push (check() == Ok): appends its actions in the order they are enqueued
    void push(int64_t n, bool host, std::vector<ChainAction> &out)
    {
        const int64_t avail = pending + n;
        if (host)
            out.push_back({ChainOp::Upload, pending, n, 0});
        accepted += n;
        const int64_t whole = avail / g.granule * g.granule;
        for (int64_t off = 0; off < whole;) {
            const int64_t p = whole - off < g.piece ? whole - off : g.piece, m = p / g.total_decimation;
            if (have - base + m > g.ring) {
                const int64_t next = frames * g.hop;
                out.push_back({ChainOp::Move, next - base, 0, have - next});
                base = next;
                moves++;
            }
            out.push_back({ChainOp::Piece, off, p, have - base});
            have += m;
            off += p;
            processed += p;
            while (have - frames * g.hop >= g.block_size) {
                const int64_t next = frames * g.hop, most = (have - next - g.block_size) / g.hop + 1;
                const int64_t f = most < g.max_batch_frames ? most : g.max_batch_frames;
                out.push_back({ChainOp::Batch, next - base, f, 0});
                frames += f;
                batches++;
            }
        }
        pending = avail - whole;
        if (host && whole > 0 && pending > 0)
            out.push_back({ChainOp::Keep, whole, 0, pending});
    }
};

}  // namespace sdr
