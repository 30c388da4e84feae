// nb.h — the impulse noise blanker's device side (include/sdrainer_hip.h "impulse noise blanker"): what capi_nb.hip holds and
// launches, implemented by k_nb.hip.  Three passes per call on the object's one stream: the blocks' powers, the gate, and
// the move of the last W powers to the front.  The integer rule is host/nb_rule.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "host/nb_rule.h"

namespace sdr {

// One workgroup of either pass owns a tile of kNbTileBytes consecutive raw bytes: four waves, each over 4 KB of its own,
// read as kNbRows loads of 16 bytes per lane, a wave's load 1 KB of consecutive input.  A block is 64 bytes (B = 64, one
// byte per sample) to 16 KB (B = 4096, sc16) and a power of two, so a tile is always whole blocks, at most kNbTileBlocks.
constexpr int kNbThreads = 256, kNbRows = 4;
constexpr int kNbTileBytes = kNbThreads * kNbRows * 16;
constexpr int kNbTileBlocks = kNbTileBytes / kNbMinBlock;
static_assert(kNbTileBytes == 16384 && kNbTileBytes == kNbMaxBlock * 4, "the largest block, 4096 sc16 samples, is one tile");
static_assert(kNbTileBlocks == kNbThreads, "a thread per block of the tile writes its power and forms its threshold");

constexpr int nb_tile_samples(int fmt) { return kNbTileBytes / ddc_sample_bytes(fmt); }
constexpr long long nb_tiles(int fmt, long long n) { return (n + nb_tile_samples(fmt) - 1) / nb_tile_samples(fmt); }

// what the device keeps between calls, besides the W powers in front of `pow`
struct NbTail {
    int open;  // the call's first `open` samples are blanked by a gate that the call before opened
    int pad;
};

struct NbLaunch {
    int fmt, block, window, ratio_q4, hold;
    const void *in;
    void *out;
    long long n;                     // samples, a positive multiple of block
    int warm;                        // the call's first `warm` blocks have fewer than W blocks behind them: not judged
    unsigned long long *pow;         // [window + n / block]: the carried powers, then the call's
    const NbTail *tail_in;           // the call before's
    NbTail *tail_out;                // this call's (the other half of the double buffer)
    uint2 *part;                     // [nb_tiles(max_in_samples)]: the gate pass's workgroups' impulses and blanked samples
    unsigned long long *rec;         // [2]: impulses, blanked, since the last read
};

hipError_t launch_nb(const NbLaunch &l, hipStream_t stream);

}  // namespace sdr
