// capi_staged.hip — the host-fed input of libsdrainer_hip.so: sdr_push_* copy the caller's frames into pinned staging
// memory, sdr_process_staged uploads what a batch needs on a copy stream and hands the float32 device rows to the
// scheduler (process_device_impl, capi_process.hip).  Three staging sets rotate (sdr_bank::StagedInput, bank.h).  What a
// band's frames can be and where their bytes lie in a set's buffers is host/staging.h; how many frames a band holds
// and what a batch leaves behind is host/overlap.h (StreamStage).  This file owns the buffers and issues the HIP calls.
#include "bank.h"

using namespace sdrcapi;
using sdr::StagedKind;
using Staging = sdr_bank::StagedInput::Staging;

namespace {

// Copy into pinned staging memory.  One core moves about 12 GB/s into write-combined-free pinned pages; a large push
// (a whole batch at once) is split over a few threads so that the copy keeps up with the PCIe upload behind it.
void staging_copy(void *dst, const void *src, size_t bytes)
{
    constexpr size_t kChunk = 8u << 20;
    const size_t parts = std::min<size_t>(bytes / kChunk, 6);
    if (parts < 2) {
        memcpy(dst, src, bytes);
        return;
    }
    std::vector<std::thread> th;
    const size_t step = ((bytes / parts) + 4095) & ~(size_t)4095;
    for (size_t i = 1; i < parts; i++) {
        const size_t off = i * step, len = (i + 1 == parts) ? bytes - off : step;
        th.emplace_back([=] { memcpy(static_cast<char *>(dst) + off, static_cast<const char *>(src) + off, len); });
    }
    memcpy(dst, src, step);
    for (auto &t : th)
        t.join();
}

// A set's buffers, each allocated at the first call that needs it.
int pinned_f32(sdr_bank *b, Staging &st)
{
    const size_t samples = b->stage_cap() * (size_t)b->cfg.n_bands;
    if (!st.h_f32)
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&st.h_f32), sizeof(float) * 2 * samples, hipHostMallocDefault));
    return SDR_OK;
}
int pinned_raw(sdr_bank *b, Staging &st)
{
    const size_t samples = b->stage_cap() * (size_t)b->cfg.n_bands;
    if (!st.h_raw)
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&st.h_raw), sizeof(int16_t) * 2 * samples, hipHostMallocDefault));
    return SDR_OK;
}
int device_f32(sdr_bank *b, Staging &st)
{
    if (!st.d_f32.p && st.d_f32.alloc(sdr::staging_buffer_bytes(false, b->stage_cap(), b->cfg.n_bands) / sizeof(float)) != hipSuccess)
        return fail(SDR_ERR_HIP, "hipMalloc iq staging failed");
    return SDR_OK;
}
int device_raw(sdr_bank *b, Staging &st)
{
    if (!st.d_raw.p && st.d_raw.alloc(sdr::staging_buffer_bytes(true, b->stage_cap(), b->cfg.n_bands)) != hipSuccess)
        return fail(SDR_ERR_HIP, "hipMalloc raw staging failed");
    return SDR_OK;
}

// the staging set the caller is filling: the copy stream, the set's events and its pinned buffer, raw or float32
int staging_ready(sdr_bank *b, bool raw)
{
    sdr_bank::StagedInput &in = b->in;
    Staging &st = in.stage[in.stage_cur];
    HIP_TRY(hipSetDevice(b->device));
    if (!in.copy_stream)
        HIP_TRY(hipStreamCreateWithFlags(&in.copy_stream, hipStreamNonBlocking));
    if (!st.uploaded) {
        HIP_TRY(hipEventCreateWithFlags(&st.uploaded, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&st.consumed, hipEventDisableTiming));
    }
    return raw ? pinned_raw(b, st) : pinned_f32(b, st);
}

// the set's pinned buffer that frames of kind `kind` are staged in
unsigned char *pinned_of(Staging &st, StagedKind kind)
{
    return sdr::staged_kind_info(kind).raw ? st.h_raw : reinterpret_cast<unsigned char *>(st.h_f32);
}

// One push of `n_values` values (two per sample) of kind `kind` behind what the band has staged.  The stream arrives in
// whole hops: at hop = block_size that is the reference's whole frames (rx/receiver.go:323-326), below it a piece is any
// whole number of hops (host/overlap.h StreamStage).
int push_samples(sdr_bank *b, int band, int sample_rate, const void *iq, size_t n_values, StagedKind kind)
{
    int rc = check_band(b, band);
    if (rc)
        return rc;
    if (!iq)
        return fail(SDR_ERR_BAD_ARG, "null iq");
    const sdr_config &c = b->cfg;
    if (sample_rate != c.sample_rate)  // rx/receiver.go:319-322
        return fail(SDR_ERR_BAD_RATE, "wrong incoming sample rate");
    const size_t per = 2 * (size_t)b->hop;
    if (n_values == 0 || n_values % per != 0)  // rx/receiver.go:323-326
        return fail(SDR_ERR_BAD_SIZE, b->hop == c.block_size ? "wrong incoming block size" : "a push must hold a whole number of hops");
    const size_t ns = n_values / 2;
    sdr_bank::StagedInput &in = b->in;
    sdr::StreamStage &ss = in.staged[band];
    if (ss.would_drop(ns, c.max_batch_frames))  // rx/receiver.go:328-333
        return fail(SDR_ERR_WOULD_DROP, "IQ data skipped: staging queue full");
    if (ss.staged > 0 && in.staged_kind[band] != kind)
        return fail(SDR_ERR_STATE, sdr::staged_kind_info(kind).mixed);
    rc = staging_ready(b, sdr::staged_kind_info(kind).raw);
    if (rc)
        return rc;
    in.staged_kind[band] = kind;
    const sdr::StagedPush at = sdr::staged_push(kind, band, b->stage_cap(), ss.staged, n_values);
    staging_copy(pinned_of(in.stage[in.stage_cur], kind) + at.offset, iq, at.bytes);  // copy on push: the caller may reuse its buffer (kiwi/client.go:203)
    ss.push(ns);
    return SDR_OK;
}

// raw frames on the device -> float32 samples, on the copy stream (k_unpack.hip)
hipError_t launch_unpack(StagedKind kind, const uint8_t *raw, float *dst, size_t n_values, hipStream_t stream)
{
    switch (kind) {
    case StagedKind::Be16: return sdr::launch_unpack_be16(raw, dst, n_values, stream);
    case StagedKind::Sc16: return sdr::launch_unpack_sc16(reinterpret_cast<const int16_t *>(raw), dst, n_values, stream);
    case StagedKind::Cs8: return sdr::launch_unpack_iq8(raw, dst, n_values, false, stream);
    case StagedKind::Cu8: return sdr::launch_unpack_iq8(raw, dst, n_values, true, stream);
    default: return hipErrorInvalidValue;  // (not a raw kind)
    }
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int sdr_push_iq(sdr_bank *b, int band, int sample_rate, const float *iq, size_t n_floats)
{
    return push_samples(b, band, sample_rate, iq, n_floats, StagedKind::F32);
}

int sdr_push_kiwi_snd(sdr_bank *b, int band, int sample_rate, const uint8_t *payload, size_t n_bytes)
{
    int rc = check_band(b, band);
    if (rc)
        return rc;
    if (b->hop != b->cfg.block_size)
        return fail(SDR_ERR_STATE, "sdr_push_kiwi_snd is not offered on a bank with hop < block_size (overlapped frames)");
    if (!payload)
        return fail(SDR_ERR_BAD_ARG, "null payload");
    if (sample_rate != b->cfg.sample_rate)
        return fail(SDR_ERR_BAD_RATE, "wrong incoming sample rate");
    constexpr size_t kHeader = 17;  // flags, sequence, S-meter, GPS (kiwi/client.go:285-290)
    const size_t per = 2 * (size_t)b->cfg.block_size * 2;  // bytes per frame: 2N int16
    if (n_bytes <= kHeader || (n_bytes - kHeader) % per != 0)  // kiwi/kiwi.go:96-98 panics on a partial block
        return fail(SDR_ERR_BAD_SIZE, "SND payload does not hold whole frames");
    return push_samples(b, band, sample_rate, payload + kHeader, (n_bytes - kHeader) / 2, StagedKind::Be16);
}

// sc16 frames from the host: staged raw like a KiwiSDR payload (half the bytes of float32 go over PCIe) and converted on
// the device by k_unpack_sc16 into the float32 staging buffer the FFT reads
int sdr_push_iq_sc16(sdr_bank *b, int band, int sample_rate, const int16_t *iq, size_t n_values)
{
    return push_samples(b, band, sample_rate, iq, n_values, StagedKind::Sc16);
}

// cs8 / cu8 frames from the host: staged raw (a quarter of the bytes of float32 go over PCIe) and converted on the device by
// k_unpack_iq8 into the float32 staging buffer the FFT reads
int sdr_push_iq8(sdr_bank *b, int band, int sample_rate, const void *iq, size_t n_values, int format)
{
    sdr::InFormat fmt;
    if (const int rc = iq8_format(format, &fmt))
        return rc;
    return push_samples(b, band, sample_rate, iq, n_values, fmt == sdr::InFormat::CU8 ? StagedKind::Cu8 : StagedKind::Cs8);
}

int sdr_staged_frames(sdr_bank *b, int band)
{
    if (check_band(b, band))
        return -1;
    return b->in.staged[band].frames();
}

int sdr_process_staged(sdr_bank *b, int *n_frames_out)
{
    return sdr_process_staged_limit(b, b ? b->cfg.max_batch_frames : 0, n_frames_out);
}

int sdr_process_staged_limit(sdr_bank *b, int max_frames, int *n_frames_out)
{
    if (!b)
        return fail(SDR_ERR_BAD_ARG, "null bank");
    const sdr_config &c = b->cfg;
    sdr_bank::StagedInput &in = b->in;
    int n = std::min(c.max_batch_frames, std::max(max_frames, 0));
    for (const sdr::StreamStage &ss : in.staged)
        n = std::min(n, ss.frames());
    if (n_frames_out)
        *n_frames_out = n;
    if (n == 0)
        return SDR_OK;
    HIP_TRY(hipSetDevice(b->device));
    const size_t cap = b->stage_cap();  // samples per band row, pinned and device alike
    const size_t span = sdr::span_samples(n, b->hop, c.block_size);
    const int prev = in.stage_cur, next = (in.stage_cur + 1) % sdr_bank::StagedInput::STAGE_RING;
    Staging &st = in.stage[prev], &nx = in.stage[next];
    int rc = device_f32(b, st);
    if (rc)
        return rc;
    // upload on the copy stream, once the FFT of this set's previous batch has read the device buffer.  Only what was
    // pushed goes up: the first `history` samples of a band's device row are already there (the batch before left them)
    HIP_TRY(hipStreamWaitEvent(in.copy_stream, st.consumed, 0));
    for (int band = 0; band < c.n_bands; band++) {
        const StagedKind kind = in.staged_kind[band];
        const sdr::StagedUpload up = sdr::staged_upload(kind, band, cap, in.staged[band].history, span);
        float *dst = st.d_f32.p + up.f32_sample * 2;
        if (sdr::staged_kind_info(kind).raw) {
            // raw int16 (KiwiSDR big-endian, or sc16) or bytes (cs8 / cu8): upload half or a quarter of the bytes, unpack in
            // HBM (k_unpack.hip)
            if ((rc = device_raw(b, st)))
                return rc;
            uint8_t *rdst = st.d_raw.p + up.raw_offset;
            HIP_TRY(hipMemcpyAsync(rdst, st.h_raw + up.src_offset, up.bytes, hipMemcpyHostToDevice, in.copy_stream));
            HIP_TRY(launch_unpack(kind, rdst, dst, up.n_values, in.copy_stream));
        } else {
            HIP_TRY(hipMemcpyAsync(dst, pinned_of(st, kind) + up.src_offset, up.bytes, hipMemcpyHostToDevice, in.copy_stream));
        }
    }
    HIP_TRY(hipEventRecord(st.uploaded, in.copy_stream));
    HIP_TRY(hipStreamWaitEvent(b->stream[S_FFT], st.uploaded, 0));
    rc = process_device_impl(b, st.d_f32.p, n, cap);
    if (rc)
        return rc;
    if (c.block_size > b->hop) {
        // The next batch's history: the last block_size - hop samples of the frames just consumed, from sample n * hop of
        // every band's row to the front of the next set's - on the FFT stream, behind this batch's FFT (which reads this
        // set) and behind the next set's last FFT (which read the rows written here; its later uploads write behind the
        // history only).
        if ((rc = device_f32(b, nx)))
            return rc;
        const sdr::StagedHistory h = sdr::staged_history(cap, (size_t)n * (size_t)b->hop, (size_t)(c.block_size - b->hop));
        HIP_TRY(hipMemcpy2DAsync(nx.d_f32.p, h.pitch, reinterpret_cast<const unsigned char *>(st.d_f32.p) + h.src_offset, h.pitch, h.width,
                                 (size_t)c.n_bands, hipMemcpyDeviceToDevice, b->stream[S_FFT]));
    }
    HIP_TRY(hipEventRecord(st.consumed, b->stream[S_FFT]));  // (behind the FFT launch and the history copy: the only readers of d_f32)
    // the caller goes on filling the next set; what this batch did not take moves to its front
    in.stage_cur = next;
    std::vector<sdr::StreamStage::Consumed> took((size_t)c.n_bands);
    bool raw = false, f32 = false;
    for (int band = 0; band < c.n_bands; band++) {
        took[(size_t)band] = in.staged[band].consume(n);
        if (took[(size_t)band].left > 0)
            (sdr::staged_kind_info(in.staged_kind[band]).raw ? raw : f32) = true;
    }
    if (f32 && (rc = staging_ready(b, false)))
        return rc;
    if (raw && (rc = staging_ready(b, true)))
        return rc;
    // the pinned buffers of the next set are free once ITS last upload has completed (two batches ago: a formality)
    if (nx.uploaded)
        HIP_TRY(hipEventSynchronize(nx.uploaded));
    for (int band = 0; band < c.n_bands; band++) {
        const StagedKind kind = in.staged_kind[band];
        if (took[(size_t)band].left > 0) {
            const sdr::StagedLeft mv = sdr::staged_left(kind, band, cap, took[(size_t)band]);
            memcpy(pinned_of(nx, kind) + mv.dst_offset, pinned_of(st, kind) + mv.src_offset, mv.bytes);
        } else {
            in.staged_kind[band] = StagedKind::None;
        }
    }
    return SDR_OK;
}

#pragma GCC visibility pop
}  // extern "C"
