// host/staging.h — the staged host input (sdr_push_* -> sdr_process_staged): what a band's staged frames can be, and
// where their bytes lie.  The one place for the kinds and for the row layout; capi_staged.hip moves the bytes.
//
// A staging set has a pinned float32 buffer, a pinned raw buffer, a float32 device buffer (what the FFT reads) and a
// raw device buffer.  Each holds one row per band of `cap` samples (what max_batch_frames frames span, host/overlap.h).
// A float32 row takes 8 bytes per sample, a raw row 4: int16 values fill it, 8-bit values half of it.  The pinned rows
// hold the samples pushed since the last batch, from the row's front; the float32 device row holds the history (the
// last block_size - hop samples of the frames the batch before consumed) and the uploaded samples behind it.
// Pure C++: tests/host/test_staging_rows.cpp moves real bytes through these very functions without a GPU.
#pragma once
#include "overlap.h"

namespace sdr {

enum class StagedKind { None, F32, Be16, Sc16, Cs8, Cu8 };  // nothing staged, float32, KiwiSDR big-endian int16, sc16, cs8, cu8

struct StagedKindInfo {
    size_t value_bytes;       // bytes per value (a sample is two values)
    size_t row_sample_bytes;  // bytes per sample of the band's row, pinned and device alike
    bool raw;                 // staged in the raw buffers and unpacked on the device (k_unpack.hip) into the float32 row
    const char *mixed;        // the refusal when the band holds frames of another kind in this batch
};

constexpr StagedKindInfo staged_kind_info(StagedKind k)
{
    switch (k) {
    case StagedKind::F32: return {4, 8, false, "band already holds int16 (KiwiSDR or sc16) or 8-bit frames in this batch"};
    case StagedKind::Be16: return {2, 4, true, "band already holds float32, sc16 or 8-bit frames in this batch"};
    case StagedKind::Sc16: return {2, 4, true, "band already holds float32, KiwiSDR or 8-bit frames in this batch"};
    case StagedKind::Cs8: return {1, 4, true, "band already holds float32, int16 or cu8 frames in this batch"};
    case StagedKind::Cu8: return {1, 4, true, "band already holds float32, int16 or cs8 frames in this batch"};
    default: return {0, 0, false, ""};
    }
}

// bytes of a set's float32 (pinned and device) or raw (pinned and device) buffer
constexpr size_t staging_buffer_bytes(bool raw, size_t cap, int n_bands) { return (raw ? 4 : 8) * cap * (size_t)n_bands; }

// byte offset of a band's row in the buffers of kind k, and bytes per staged sample of that kind
constexpr size_t staged_row_offset(StagedKind k, int band, size_t cap) { return (size_t)band * cap * staged_kind_info(k).row_sample_bytes; }
constexpr size_t staged_sample_bytes(StagedKind k) { return 2 * staged_kind_info(k).value_bytes; }

// A push of n_values values behind the `staged` samples (StreamStage::staged) the band holds: where it lands in the set's
// pinned buffer of its kind, and how many bytes it is.
struct StagedPush {
    size_t offset, bytes;
};
constexpr StagedPush staged_push(StagedKind k, int band, size_t cap, size_t staged, size_t n_values)
{
    return {staged_row_offset(k, band, cap) + staged * staged_sample_bytes(k), n_values * staged_kind_info(k).value_bytes};
}

// What a batch whose frames span `span` samples uploads for a band that has `history` samples on the device already
// (StreamStage::history): `bytes` from `src_offset` of the pinned buffer of its kind - for a raw kind to `raw_offset` of the
// raw device buffer, where the unpack kernel reads `n_values` values - to sample `f32_sample` of the float32 device buffer.
struct StagedUpload {
    size_t src_offset, bytes, raw_offset, f32_sample, n_values;
};
constexpr StagedUpload staged_upload(StagedKind k, int band, size_t cap, size_t history, size_t span)
{
    const size_t up = span - history;  // samples (StreamStage::Consumed::uploaded)
    return {staged_row_offset(k, band, cap), up * staged_sample_bytes(k), staged_row_offset(k, band, cap), (size_t)band * cap + history, 2 * up};
}

// The next batch's history: the last `overlap` samples of the frames just consumed, from sample `keep_from`
// (StreamStage::Consumed) of every band's float32 device row to the front of the next set's - one 2D copy of `width`
// bytes per row, `src_offset` into the first row, rows `pitch` bytes apart.
struct StagedHistory {
    size_t src_offset, width, pitch;
};
constexpr StagedHistory staged_history(size_t cap, size_t keep_from, size_t overlap) { return {keep_from * 8, overlap * 8, cap * 8}; }

// What a batch did not take moves to the front of the band's row in the next set's pinned buffer of its kind.
struct StagedLeft {
    size_t src_offset, dst_offset, bytes;
};
constexpr StagedLeft staged_left(StagedKind k, int band, size_t cap, const StreamStage::Consumed &t)
{
    return {staged_row_offset(k, band, cap) + t.left_from * staged_sample_bytes(k), staged_row_offset(k, band, cap), t.left * staged_sample_bytes(k)};
}

}  // namespace sdr
