// capi_nb.hip — the impulse noise blanker behind the C ABI (include/sdrainer_hip.h "impulse noise blanker"): an object of its
// own in front of the DDC, the channelizer or the bank, raw samples in and raw samples of the same format out, both in device
// memory.  The passes are k_nb.hip's, the integer rule host/nb_rule.h's.
//
// Between calls the device keeps the last W block powers in front of the powers' array, the open gate's remaining length
// (NbTail, double-buffered: a call's gate pass reads tail[cur] and its last workgroup writes tail[1 - cur]) and the two
// counts, which the carry pass adds up from one row per workgroup of the gate pass.  The host keeps only counters.
// Everything is ordered by the blanker's one stream; no call waits for the device.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "nb.h"

namespace sdr {
int set_error(int code, const char *msg);  // capi_bank.hip: feeds sdr_last_error()
}

namespace {

int nfail(int code, const std::string &msg) { return sdr::set_error(code, msg.c_str()); }
#define NHIP(expr)                                                                          \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return nfail(SDR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

size_t sample_bytes(int fmt) { return (size_t)sdr::ddc_sample_bytes(fmt); }

int check_config(const sdr_nb_config *cfg)
{
    if (cfg->struct_size != (int32_t)sizeof(sdr_nb_config))
        return nfail(SDR_ERR_BAD_ARG, "sdr_nb_config.struct_size mismatch");
    if (!sdr::nb_format(cfg->in_format))
        return nfail(SDR_ERR_BAD_ARG, "in_format must be SDR_DDC_SC16, _CS8, _CU8, _RS16, _RS8 or _RU8 (float32 streams are not blanked)");
    if (!sdr::nb_geometry(cfg->block, cfg->window))
        return nfail(SDR_ERR_BAD_ARG, "block must be a power of two in 64 .. 4096, window one in 1 .. 64, block * window <= 65536");
    if (!sdr::nb_threshold_valid(cfg->block, cfg->ratio_q4, cfg->hold))
        return nfail(SDR_ERR_BAD_ARG, "ratio_q4 must be 0 or 16 .. 16384, hold 0 .. block");
    if (cfg->max_in_samples < cfg->block || cfg->max_in_samples % cfg->block != 0)
        return nfail(SDR_ERR_BAD_ARG, "max_in_samples must be a positive multiple of block");
    return SDR_OK;
}

}  // namespace

struct sdr_nb {
    sdr_nb_config cfg{};
    hipStream_t stream = nullptr;
    int ratio_q4 = 0, hold = 0;  // current: sdr_nb_set_threshold
    unsigned long long *d_pow = nullptr;  // [window + max_in_samples / block]
    sdr::NbTail *d_tail = nullptr;        // [2]
    unsigned long long *d_rec = nullptr;  // [2]: impulses, blanked
    uint2 *d_part = nullptr;              // [tiles of max_in_samples]: one call's counts per workgroup of the gate pass
    int cur = 0;                          // the tail the next call reads
    int64_t origin = 0, total = 0;        // index of the first and of the next sample
    int64_t seen = 0;                     // samples since the last read of the statistics
    bool started = false;
    // sdr_nb_process_host: the upload, through pinned memory (allocated by the first such call)
    void *h_pin = nullptr, *d_in = nullptr;
    hipEvent_t uploaded = nullptr;
};

namespace sdr {
const sdr_nb_config &nb_config(const sdr_nb *nb) { return nb->cfg; }  // chain.h
hipStream_t nb_stream(const sdr_nb *nb) { return nb->stream; }
}

namespace {

int check_call(sdr_nb *nb, const void *in, size_t n_in, const void *out, bool in_on_device)
{
    if (!nb || !in || !out)
        return nfail(SDR_ERR_BAD_ARG, "null blanker, input or output");
    const size_t B = (size_t)nb->cfg.block;
    if (n_in == 0 || n_in % B != 0 || n_in > (size_t)nb->cfg.max_in_samples)
        return nfail(SDR_ERR_BAD_SIZE, "n_in_samples must be a positive multiple of block, at most max_in_samples");
    if ((in_on_device && ((uintptr_t)in & 15u)) || ((uintptr_t)out & 15u))
        return nfail(SDR_ERR_BAD_ARG, "in_dev and out_dev must be 16-byte aligned");
    const uintptr_t bytes = sample_bytes(nb->cfg.in_format) * n_in, a = (uintptr_t)in, o = (uintptr_t)out;
    if (in_on_device && a < o + bytes && o < a + bytes)
        return nfail(SDR_ERR_BAD_ARG, "in_dev and out_dev must not overlap (the gate reads samples in front of the ones it writes)");
    return SDR_OK;
}

int run(sdr_nb *nb, const void *in_dev, size_t n_in, void *out_dev)
{
    const sdr_nb_config &c = nb->cfg;
    const int64_t blocks_behind = (nb->total - nb->origin) / c.block;
    sdr::NbLaunch l{};
    l.fmt = c.in_format;
    l.block = c.block;
    l.window = c.window;
    l.ratio_q4 = nb->ratio_q4;
    l.hold = nb->hold;
    l.in = in_dev;
    l.out = out_dev;
    l.n = (long long)n_in;
    l.warm = blocks_behind >= c.window ? 0 : (int)(c.window - blocks_behind);
    l.pow = nb->d_pow;
    l.tail_in = nb->d_tail + nb->cur;
    l.tail_out = nb->d_tail + (1 - nb->cur);
    l.part = nb->d_part;
    l.rec = nb->d_rec;
    NHIP(sdr::launch_nb(l, nb->stream));
    nb->cur = 1 - nb->cur;
    nb->total += (int64_t)n_in;
    nb->seen += (int64_t)n_in;
    nb->started = true;
    return SDR_OK;
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int sdr_nb_destroy(sdr_nb *nb)
{
    if (!nb)
        return SDR_OK;
    (void)hipSetDevice(nb->cfg.device_id);
    (void)hipStreamSynchronize(nb->stream);
    (void)hipFree(nb->d_pow);
    (void)hipFree(nb->d_tail);
    (void)hipFree(nb->d_rec);
    (void)hipFree(nb->d_part);
    (void)hipFree(nb->d_in);
    if (nb->h_pin)
        (void)hipHostFree(nb->h_pin);
    if (nb->uploaded)
        (void)hipEventDestroy(nb->uploaded);
    delete nb;
    return SDR_OK;
}

int sdr_nb_create(const sdr_nb_config *cfg, sdr_nb **out)
{
    if (!cfg || !out)
        return nfail(SDR_ERR_BAD_ARG, "null config or output");
    const int rc = check_config(cfg);
    if (rc)
        return rc;
    NHIP(hipSetDevice(cfg->device_id));
    sdr_nb *nb = new sdr_nb();
    nb->cfg = *cfg;
    nb->ratio_q4 = cfg->ratio_q4;
    nb->hold = cfg->hold;
    // (a failure half way frees what was allocated so far: sdr_nb_destroy tolerates null members)
#define NCREATE(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            const std::string _msg = std::string(#expr) + ": " + hipGetErrorString(_e);     \
            sdr_nb_destroy(nb);                                                             \
            return nfail(SDR_ERR_HIP, _msg);                                                \
        }                                                                                   \
    } while (0)
    const size_t pow_bytes = sizeof(unsigned long long) * ((size_t)cfg->window + (size_t)(cfg->max_in_samples / cfg->block));
    NCREATE(hipMalloc((void **)&nb->d_pow, pow_bytes));
    NCREATE(hipMemset(nb->d_pow, 0, pow_bytes));
    NCREATE(hipMalloc((void **)&nb->d_tail, 2 * sizeof(sdr::NbTail)));
    NCREATE(hipMemset(nb->d_tail, 0, 2 * sizeof(sdr::NbTail)));
    NCREATE(hipMalloc((void **)&nb->d_rec, 2 * sizeof(unsigned long long)));
    NCREATE(hipMemset(nb->d_rec, 0, 2 * sizeof(unsigned long long)));
    NCREATE(hipMalloc((void **)&nb->d_part, sizeof(uint2) * (size_t)sdr::nb_tiles(cfg->in_format, cfg->max_in_samples)));
#undef NCREATE
    *out = nb;
    return SDR_OK;
}

int sdr_nb_sync(sdr_nb *nb)
{
    if (!nb)
        return nfail(SDR_ERR_BAD_ARG, "null blanker");
    NHIP(hipSetDevice(nb->cfg.device_id));
    NHIP(hipStreamSynchronize(nb->stream));
    return SDR_OK;
}

int sdr_nb_set_stream(sdr_nb *nb, void *hip_stream)
{
    if (!nb)
        return nfail(SDR_ERR_BAD_ARG, "null blanker");
    NHIP(hipSetDevice(nb->cfg.device_id));
    NHIP(hipStreamSynchronize(nb->stream));  // (the state of the calls so far is ordered by the old stream)
    nb->stream = (hipStream_t)hip_stream;
    return SDR_OK;
}

int sdr_nb_set_first_sample(sdr_nb *nb, int64_t k0)
{
    if (!nb)
        return nfail(SDR_ERR_BAD_ARG, "null blanker");
    if (nb->started)
        return nfail(SDR_ERR_STATE, "sdr_nb_set_first_sample: the blanker has processed samples (call it right after sdr_nb_create)");
    if (k0 < 0 || k0 % nb->cfg.block != 0)
        return nfail(SDR_ERR_BAD_ARG, "the first sample must be >= 0 and a multiple of block");
    nb->origin = nb->total = k0;
    return SDR_OK;
}

int64_t sdr_nb_total_samples(sdr_nb *nb) { return nb ? nb->total : 0; }

int sdr_nb_set_threshold(sdr_nb *nb, int ratio_q4, int hold)
{
    if (!nb)
        return nfail(SDR_ERR_BAD_ARG, "null blanker");
    if (!sdr::nb_threshold_valid(nb->cfg.block, ratio_q4, hold))
        return nfail(SDR_ERR_BAD_ARG, "ratio_q4 must be 0 or 16 .. 16384, hold 0 .. block");
    nb->ratio_q4 = ratio_q4;
    nb->hold = hold;
    return SDR_OK;
}

int sdr_nb_process_device(sdr_nb *nb, const void *in_dev, size_t n_in_samples, void *out_dev)
{
    const int rc = check_call(nb, in_dev, n_in_samples, out_dev, true);
    if (rc)
        return rc;
    NHIP(hipSetDevice(nb->cfg.device_id));
    return run(nb, in_dev, n_in_samples, out_dev);
}

int sdr_nb_process_host(sdr_nb *nb, const void *in_host, size_t n_in_samples, void *out_dev)
{
    const int rc = check_call(nb, in_host, n_in_samples, out_dev, false);
    if (rc)
        return rc;
    NHIP(hipSetDevice(nb->cfg.device_id));
    const size_t cap = sample_bytes(nb->cfg.in_format) * (size_t)nb->cfg.max_in_samples;
    if (!nb->d_in)
        NHIP(hipMalloc(&nb->d_in, cap));
    if (!nb->h_pin)
        NHIP(hipHostMalloc(&nb->h_pin, cap, hipHostMallocDefault));
    if (!nb->uploaded)
        NHIP(hipEventCreateWithFlags(&nb->uploaded, hipEventDisableTiming));
    else
        NHIP(hipEventSynchronize(nb->uploaded));  // the pinned buffer is free once the last upload has left it
    const size_t bytes = sample_bytes(nb->cfg.in_format) * n_in_samples;
    const uintptr_t a = (uintptr_t)nb->d_in, o = (uintptr_t)out_dev;
    if (a < o + bytes && o < a + bytes)
        return nfail(SDR_ERR_BAD_ARG, "out_dev overlaps the blanker's own upload buffer");
    memcpy(nb->h_pin, in_host, bytes);
    NHIP(hipMemcpyAsync(nb->d_in, nb->h_pin, bytes, hipMemcpyHostToDevice, nb->stream));
    NHIP(hipEventRecord(nb->uploaded, nb->stream));
    return run(nb, nb->d_in, n_in_samples, out_dev);
}

int sdr_nb_read_stats(sdr_nb *nb, sdr_nb_stats *out)
{
    if (!nb || !out)
        return nfail(SDR_ERR_BAD_ARG, "null blanker or output");
    NHIP(hipSetDevice(nb->cfg.device_id));
    unsigned long long rec[2];
    NHIP(hipMemcpyAsync(rec, nb->d_rec, sizeof rec, hipMemcpyDeviceToHost, nb->stream));
    NHIP(hipStreamSynchronize(nb->stream));
    NHIP(hipMemsetAsync(nb->d_rec, 0, sizeof rec, nb->stream));
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
        return nfail(SDR_ERR_BAD_ARG, "null config, input or output");
    const int rc = check_config(cfg);
    if (rc)
        return rc;
    if (n_in_samples == 0 || n_in_samples % (size_t)cfg->block != 0)
        return nfail(SDR_ERR_BAD_SIZE, "n_in_samples must be a positive multiple of block");
    const uintptr_t bytes = sample_bytes(cfg->in_format) * n_in_samples, a = (uintptr_t)in, o = (uintptr_t)out;
    if (a < o + bytes && o < a + bytes)
        return nfail(SDR_ERR_BAD_ARG, "in and out must not overlap");
    const sdr::NbTotals t = sdr::nb_blank_stream_host(cfg->in_format, cfg->block, cfg->window, cfg->ratio_q4, cfg->hold, in, n_in_samples, out);
    if (stats)
        *stats = sdr_nb_stats{(int64_t)n_in_samples, t.impulses, t.blanked, 0};
    return SDR_OK;
}

#pragma GCC visibility pop
}
