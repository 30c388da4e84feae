// test_chain_plan.cpp — the receive chain's plan (csrc/host/chain_plan.h) over seeded random geometries and push lengths, every
// action printed: tests/test_chain_plan.py builds this program with -fsanitize=address,undefined, compares its output line
// for line with tests/chain_ref.py's trace() and checks the invariants on it.  The generator and the order of the draws are
// chain_ref.py's (SplitMix, draw_geometry, draw_push).  No HIP, no GPU.
//   usage: test_chain_plan [seed geometries pushes]
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sdrainer_amd/csrc/host/chain_plan.h"

namespace {

struct SplitMix {
    uint64_t s;
    uint64_t next()
    {
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    int64_t below(int64_t n) { return (int64_t)(next() % (uint64_t)n); }
};

const int64_t kDtots[] = {1, 2, 3, 5, 8, 12, 32, 100, 256, 1000, 4096, 8192};
const int64_t kNbBlocks[] = {1, 64, 96, 256, 4096};
const int64_t kMaxBatch[] = {3, 7, 64, 1024};

const char *name(sdr::ChainOp op)
{
    switch (op) {
    case sdr::ChainOp::Upload: return "upload";
    case sdr::ChainOp::Piece: return "piece";
    case sdr::ChainOp::Move: return "move";
    case sdr::ChainOp::Batch: return "batch";
    case sdr::ChainOp::Keep: return "keep";
    }
    return "?";
}

}  // namespace

int main(int argc, char **argv)
{
    SplitMix rng{argc > 1 ? strtoull(argv[1], nullptr, 10) : 20250117ull};
    const int geometries = argc > 2 ? atoi(argv[2]) : 160, pushes = argc > 3 ? atoi(argv[3]) : 48;
    std::vector<sdr::ChainAction> actions;
    for (int i = 0; i < geometries; i++) {
        sdr::ChainPlan plan;
        sdr::ChainGeometry &g = plan.g;
        g.block_size = int64_t(512) << rng.below(5);
        g.hop = g.block_size >> rng.below(5);
        g.total_decimation = rng.below(2) ? kDtots[rng.below(12)] : 1 + rng.below(8192);
        const int64_t nb = kNbBlocks[rng.below(5)];
        g.granule = sdr::chain_granule(g.total_decimation, nb);
        const int64_t limit = g.granule * (1 + rng.below(6)) + rng.below(g.granule);
        g.piece = sdr::chain_piece(g.granule, limit);
        g.max_in = 1 + rng.below(3 * g.piece + 17);
        g.max_batch_frames = kMaxBatch[rng.below(4)];
        g.ring = sdr::chain_min_ring(g.block_size, g.hop, g.piece, g.total_decimation);
        if (rng.below(2))
            g.ring += 4 * rng.below(g.ring / 2);
        printf("geom %d dtot %" PRId64 " nb %" PRId64 " granule %" PRId64 " piece %" PRId64 " ring %" PRId64 " block %" PRId64 " hop %" PRId64
               " max_batch %" PRId64 " max_in %" PRId64 "\n",
               i, g.total_decimation, nb, g.granule, g.piece, g.ring, g.block_size, g.hop, g.max_batch_frames, g.max_in);
        for (int k = 0; k < pushes; k++) {
            const int64_t kind = rng.below(8);
            int64_t n;
            bool host = true;
            if (kind < 2) {
                const int64_t most = g.max_in / g.granule;
                n = g.granule * (1 + rng.below(most > 1 ? most : 1));
                host = false;
            } else if (kind == 2) {
                n = 1;
            } else if (kind == 3) {
                n = 1 + rng.below(g.granule);
            } else if (kind == 4) {
                n = g.max_in;
            } else {
                n = 1 + rng.below(g.max_in);
            }
            printf("push %" PRId64 " %s\n", n, host ? "host" : "device");
            const sdr::ChainPlan::Refusal why = plan.check(n, host);
            if (why != sdr::ChainPlan::Ok) {
                printf("refuse %s\n", why == sdr::ChainPlan::BadSize ? "size" : "state");
                continue;
            }
            actions.clear();
            plan.push(n, host, actions);
            for (const sdr::ChainAction &a : actions) {
                if (a.op == sdr::ChainOp::Upload || a.op == sdr::ChainOp::Batch)
                    printf("%s %" PRId64 " %" PRId64 "\n", name(a.op), a.a, a.b);
                else
                    printf("%s %" PRId64 " %" PRId64 " %" PRId64 "\n", name(a.op), a.a, a.b, a.c);
            }
            printf("state %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", plan.accepted,
                   plan.processed, plan.pending, plan.base, plan.have, plan.frames, plan.batches, plan.moves);
        }
    }
    return 0;
}
