// host/overlap.h — overlapped frames: frame f of a band starts at sample f * hop of the band's stream, hop <= block_size.
// Three small things every layer shares, in one place:
//   - the index function of the FFT kernels' input (band, frame, strides) -> sample offset;
//   - which hops sdr_create accepts;
//   - the arithmetic of the staged host input: how many complete frames a band's stream holds, what a batch consumes and
//     which samples stay behind as the next batch's history.
// Pure C++ (SDR_HD where a kernel calls it): tests/host/test_overlap_staging.cpp runs these very functions without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SDR_HD __host__ __device__
#else
#define SDR_HD
#endif

namespace sdr {

// Sample offset of frame `frame` of a band whose stream starts `band_base` samples into the input: what every FFT input
// path adds to the input pointer (times two floats or int16 values).  Dense frames are frame_stride == block_size.
SDR_HD inline size_t input_sample_offset(size_t band_base, unsigned frame, int frame_stride)
{
    return band_base + (size_t)frame * (size_t)(unsigned)frame_stride;
}

// sdr_config.hop as sdr_create takes it: 0 = block_size; else a power of two, block_size / 16 <= hop <= block_size and
// hop >= 32 (a frame start stays 16-byte aligned in sc16, 4 bytes per sample, as well)
inline bool hop_valid(int hop, int block_size)
{
    if (hop == 0)
        return true;
    if (hop < 32 || hop > block_size || (hop & (hop - 1)) != 0)
        return false;
    return (long long)hop * 16 >= block_size;
}
inline int effective_hop(int hop, int block_size) { return hop == 0 ? block_size : hop; }

// Samples per band that n_frames overlapped frames span (0 frames: none)
inline size_t span_samples(int n_frames, int hop, int block_size)
{
    return n_frames > 0 ? (size_t)(n_frames - 1) * (size_t)hop + (size_t)block_size : 0;
}

// One band's staged stream.  `history` samples kept from the batch before (0 before the first batch, block_size - hop
// after it) sit in front of `staged` samples pushed since.  Everything counts samples.
struct StreamStage {
    int block_size = 0, hop = 0;
    size_t history = 0, staged = 0;

    size_t overlap() const { return (size_t)(block_size - hop); }
    // complete frames: max(0, (history + staged - (block_size - hop)) / hop)
    int frames() const
    {
        const size_t have = history + staged;
        return have < overlap() ? 0 : (int)((have - overlap()) / (size_t)hop);
    }
    // samples a band may hold: what max_batch_frames frames span
    size_t capacity(int max_batch_frames) const { return span_samples(max_batch_frames, hop, block_size); }
    // would `n` more samples overflow the staging set (SDR_ERR_WOULD_DROP)?
    bool would_drop(size_t n, int max_batch_frames) const { return history + staged + n > capacity(max_batch_frames); }
    void push(size_t n) { staged += n; }
    // A batch of n frames (n <= frames()) reads samples [0, span) of history + staged.  Afterwards the stream continues
    // at sample n * hop: its first block_size - hop samples are the next batch's history (on the device already), the
    // rest is what was pushed and not yet consumed (`left`, the tail of the staged samples, moves to the next set).
    struct Consumed {
        size_t uploaded;    // staged samples the batch needed on the device: span - history
        size_t keep_from;   // sample (of history + staged) the new history starts at: n * hop
        size_t left_from;   // first staged sample (index into the staged part) that stays staged
        size_t left;        // how many stay staged
    };
    Consumed consume(int n)
    {
        Consumed c{};
        if (n <= 0)
            return c;
        const size_t span = span_samples(n, hop, block_size);
        c.uploaded = span - history;
        c.keep_from = (size_t)n * (size_t)hop;
        c.left_from = c.uploaded;
        c.left = staged - c.uploaded;
        history = overlap();
        staged = c.left;
        return c;
    }
};

}  // namespace sdr
