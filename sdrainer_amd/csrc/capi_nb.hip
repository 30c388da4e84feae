// capi_nb.hip — the impulse noise blanker behind the C ABI (include/sdrainer_hip.h "impulse noise blanker"): an object of its
// own in front of the DDC, the channelizer or the bank, raw samples in and raw samples of the same format out, both in device
// memory.  The passes are k_nb.hip's, the integer rule host/nb_rule.h's.
//
// Between calls the device keeps the last W block powers in front of the powers' array, the open gate's remaining length
// (NbTail, double-buffered: a call's gate pass reads tail[cur] and its last workgroup writes tail[1 - cur]) and the two
// counts, which the carry pass adds up from one row per workgroup of the gate pass.  The host keeps only counters.
// Everything is ordered by the blanker's one stream; no call waits for the device.  The stream, the sample clock (its unit
// is the block), process_host's upload and the first checks of a call are front.h's.
#include "front.h"
#include "nb.h"

using sdr::fail;

namespace {

size_t sample_bytes(int fmt) { return (size_t)sdr::ddc_sample_bytes(fmt); }

int check_config(const sdr_nb_config *cfg)
{
    if (cfg->struct_size != (int32_t)sizeof(sdr_nb_config))
        return fail(SDR_ERR_BAD_ARG, "sdr_nb_config.struct_size mismatch");
    if (!sdr::nb_format(cfg->in_format))
        return fail(SDR_ERR_BAD_ARG, "in_format must be SDR_DDC_SC16, _CS8, _CU8, _RS16, _RS8 or _RU8 (float32 streams are not blanked)");
    if (!sdr::nb_geometry(cfg->block, cfg->window))
        return fail(SDR_ERR_BAD_ARG, "block must be a power of two in 64 .. 4096, window one in 1 .. 64, block * window <= 65536");
    if (!sdr::nb_threshold_valid(cfg->block, cfg->ratio_q4, cfg->hold))
        return fail(SDR_ERR_BAD_ARG, "ratio_q4 must be 0 or 16 .. 16384, hold 0 .. block");
    if (cfg->max_in_samples < cfg->block || cfg->max_in_samples % cfg->block != 0)
        return fail(SDR_ERR_BAD_ARG, "max_in_samples must be a positive multiple of block");
    return SDR_OK;
}

}  // namespace

struct sdr_nb : sdr::FrontObject {
    sdr_nb_config cfg{};
    int ratio_q4 = 0, hold = 0;  // current: sdr_nb_set_threshold
    unsigned long long *d_pow = nullptr;  // [window + max_in_samples / block]
    sdr::NbTail *d_tail = nullptr;        // [2]
    unsigned long long *d_rec = nullptr;  // [2]: impulses, blanked
    uint2 *d_part = nullptr;              // [tiles of max_in_samples]: one call's counts per workgroup of the gate pass
    int cur = 0;                          // the tail the next call reads
    int64_t seen = 0;                     // samples since the last read of the statistics
    sdr::HostUpload upload;               // sdr_nb_process_host
};

namespace sdr {
const sdr_nb_config &nb_config(const sdr_nb *nb) { return nb->cfg; }  // chain.h
hipStream_t nb_stream(const sdr_nb *nb) { return nb->stream; }
}

namespace {

const sdr::CallTexts kCall = {"null blanker, input or output", "n_in_samples must be a positive multiple of block, at most max_in_samples",
                              "in_dev and out_dev must be 16-byte aligned"};

int check_call(sdr_nb *nb, const void *in, size_t n_in, const void *out, bool in_on_device)
{
    const int rc = sdr::check_call(nb, in, n_in, out, in_on_device, kCall);
    if (rc)
        return rc;
    if (in_on_device && sdr::ranges_overlap(in, out, sdr::span_bytes(sdr::ddc_sample_bytes(nb->cfg.in_format), n_in)))
        return fail(SDR_ERR_BAD_ARG, "in_dev and out_dev must not overlap (the gate reads samples in front of the ones it writes)");
    return SDR_OK;
}

int run(sdr_nb *nb, const void *in_dev, size_t n_in, void *out_dev)
{
    const sdr_nb_config &c = nb->cfg;
    sdr::NbLaunch l{};
    l.fmt = c.in_format;
    l.block = c.block;
    l.window = c.window;
    l.ratio_q4 = nb->ratio_q4;
    l.hold = nb->hold;
    l.in = in_dev;
    l.out = out_dev;
    l.n = (long long)n_in;
    l.warm = nb->clock.warm_blocks(c.window);
    l.pow = nb->d_pow;
    l.tail_in = nb->d_tail + nb->cur;
    l.tail_out = nb->d_tail + (1 - nb->cur);
    l.part = nb->d_part;
    l.rec = nb->d_rec;
    HIP_TRY(sdr::launch_nb(l, nb->stream));
    nb->cur = 1 - nb->cur;
    nb->clock.advance(n_in);
    nb->seen += (int64_t)n_in;
    return SDR_OK;
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int sdr_nb_destroy(sdr_nb *nb)
{
    if (!nb)
        return SDR_OK;
    nb->quiesce();
    (void)hipFree(nb->d_pow);
    (void)hipFree(nb->d_tail);
    (void)hipFree(nb->d_rec);
    (void)hipFree(nb->d_part);
    nb->upload.release();
    delete nb;
    return SDR_OK;
}

int sdr_nb_create(const sdr_nb_config *cfg, sdr_nb **out)
{
    if (!cfg || !out)
        return fail(SDR_ERR_BAD_ARG, "null config or output");
    const int rc = check_config(cfg);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(cfg->device_id));
    sdr::Building<sdr_nb, sdr_nb_destroy> nb(new sdr_nb());
    nb->cfg = *cfg;
    nb->place(cfg->device_id, cfg->block, cfg->max_in_samples);
    nb->ratio_q4 = cfg->ratio_q4;
    nb->hold = cfg->hold;
    const size_t pow_bytes = sizeof(unsigned long long) * ((size_t)cfg->window + (size_t)(cfg->max_in_samples / cfg->block));
    HIP_TRY(hipMalloc((void **)&nb->d_pow, pow_bytes));
    HIP_TRY(hipMemset(nb->d_pow, 0, pow_bytes));
    HIP_TRY(hipMalloc((void **)&nb->d_tail, 2 * sizeof(sdr::NbTail)));
    HIP_TRY(hipMemset(nb->d_tail, 0, 2 * sizeof(sdr::NbTail)));
    HIP_TRY(hipMalloc((void **)&nb->d_rec, 2 * sizeof(unsigned long long)));
    HIP_TRY(hipMemset(nb->d_rec, 0, 2 * sizeof(unsigned long long)));
    HIP_TRY(hipMalloc((void **)&nb->d_part, sizeof(uint2) * (size_t)sdr::nb_tiles(cfg->in_format, cfg->max_in_samples)));
    *out = nb.release();
    return SDR_OK;
}

int sdr_nb_sync(sdr_nb *nb) { return sdr::front_sync(nb, "null blanker"); }

int sdr_nb_set_stream(sdr_nb *nb, void *hip_stream) { return sdr::front_set_stream(nb, hip_stream, "null blanker"); }

int sdr_nb_set_first_sample(sdr_nb *nb, int64_t k0)
{
    return sdr::front_set_first_sample(nb, k0, "null blanker",
                                       "sdr_nb_set_first_sample: the blanker has processed samples (call it right after sdr_nb_create)",
                                       "the first sample must be >= 0 and a multiple of block");
}

int64_t sdr_nb_total_samples(sdr_nb *nb) { return sdr::front_total_samples(nb); }

int sdr_nb_set_threshold(sdr_nb *nb, int ratio_q4, int hold)
{
    if (!nb)
        return fail(SDR_ERR_BAD_ARG, "null blanker");
    if (!sdr::nb_threshold_valid(nb->cfg.block, ratio_q4, hold))
        return fail(SDR_ERR_BAD_ARG, "ratio_q4 must be 0 or 16 .. 16384, hold 0 .. block");
    nb->ratio_q4 = ratio_q4;
    nb->hold = hold;
    return SDR_OK;
}

int sdr_nb_process_device(sdr_nb *nb, const void *in_dev, size_t n_in_samples, void *out_dev)
{
    const int rc = check_call(nb, in_dev, n_in_samples, out_dev, true);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(nb->device_id));
    return run(nb, in_dev, n_in_samples, out_dev);
}

int sdr_nb_process_host(sdr_nb *nb, const void *in_host, size_t n_in_samples, void *out_dev)
{
    int rc = check_call(nb, in_host, n_in_samples, out_dev, false);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(nb->device_id));
    const size_t sb = sample_bytes(nb->cfg.in_format), bytes = sdr::span_bytes((int)sb, n_in_samples);
    // (the upload's two halves apart: the overlap can be judged only once the upload buffer exists)
    if ((rc = nb->upload.ready(sb * (size_t)nb->cfg.max_in_samples, true)))
        return rc;
    if (sdr::ranges_overlap(nb->upload.d_in, out_dev, bytes))
        return fail(SDR_ERR_BAD_ARG, "out_dev overlaps the blanker's own upload buffer");
    if ((rc = nb->upload.send(in_host, bytes, nb->upload.d_in, nb->stream)))
        return rc;
    return run(nb, nb->upload.d_in, n_in_samples, out_dev);
}

int sdr_nb_read_stats(sdr_nb *nb, sdr_nb_stats *out)
{
    if (!nb || !out)
        return fail(SDR_ERR_BAD_ARG, "null blanker or output");
    HIP_TRY(hipSetDevice(nb->device_id));
    unsigned long long rec[2];
    HIP_TRY(hipMemcpyAsync(rec, nb->d_rec, sizeof rec, hipMemcpyDeviceToHost, nb->stream));
    HIP_TRY(hipStreamSynchronize(nb->stream));
    HIP_TRY(hipMemsetAsync(nb->d_rec, 0, sizeof rec, nb->stream));
    *out = sdr_nb_stats{nb->seen, (int64_t)rec[0], (int64_t)rec[1], 0};
    nb->seen = 0;
    return SDR_OK;
}

int sdr_nb_tile_samples(int in_format, int block)
{
    if (!sdr::nb_format(in_format) || !sdr::nb_geometry(block, 1))
        return -1;
    return sdr::nb_tile_samples(in_format);
}

int sdr_nb_blank_host(const sdr_nb_config *cfg, const void *in, size_t n_in_samples, void *out, sdr_nb_stats *stats)
{
    if (!cfg || !in || !out)
        return fail(SDR_ERR_BAD_ARG, "null config, input or output");
    const int rc = check_config(cfg);
    if (rc)
        return rc;
    if (n_in_samples == 0 || n_in_samples % (size_t)cfg->block != 0)
        return fail(SDR_ERR_BAD_SIZE, "n_in_samples must be a positive multiple of block");
    if (sdr::ranges_overlap(in, out, sample_bytes(cfg->in_format) * n_in_samples))  // (no max_in_samples bounds this stream)
        return fail(SDR_ERR_BAD_ARG, "in and out must not overlap");
    const sdr::NbTotals t = sdr::nb_blank_stream_host(cfg->in_format, cfg->block, cfg->window, cfg->ratio_q4, cfg->hold, in, n_in_samples, out);
    if (stats)
        *stats = sdr_nb_stats{(int64_t)n_in_samples, t.impulses, t.blanked, 0};
    return SDR_OK;
}

#pragma GCC visibility pop
}
