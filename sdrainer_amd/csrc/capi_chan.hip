// capi_chan.hip — the polyphase channelizer behind the C ABI (include/sdrainer_hip.h "channelizer"): an object of its own
// beside the bank and the down-converter, with the taps, the table of twiddles, the channel list and the carry of n_taps - 1
// raw samples in device memory.  The kernel is k_chan.h, instantiated by k_chan.hip; a sample's size is host/ddc_format.h's.
//
// The carry is the down-converter's (capi_ddc.hip): double-buffered, formed by launch_ddc_carry behind each call's kernel,
// everything ordered by the channelizer's one stream.  The IQ correction and the raw stream's sums are the down-converter's
// too: k_chan_iqc.hip's instance while a correction is set, k_iq_sums.hip behind the carry's kernel with the sums on.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "chan.h"
#include "ddc.h"
#include "host/ddc_format.h"
#include "iq_sums_dev.h"
#include "host/nco_table.h"

namespace sdr {
int set_error(int code, const char *msg);  // capi_bank.hip: feeds sdr_last_error()
}

namespace {

int cfail(int code, const std::string &msg) { return sdr::set_error(code, msg.c_str()); }
#define CHIP(expr)                                                                          \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return cfail(SDR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

size_t sample_bytes(int fmt) { return (size_t)sdr::ddc_sample_bytes(fmt); }  // 8, 4, 2 complex; 4, 2, 1 real

}  // namespace

struct sdr_chan {
    sdr_chan_config cfg{};
    hipStream_t stream = nullptr;
    float *d_taps = nullptr;
    float2 *d_nco = nullptr;
    int *d_channels = nullptr;
    void *d_carry[2] = {nullptr, nullptr};
    int cur = 0;            // the carry buffer the next call reads
    int64_t origin = 0;     // index of the channelizer's first sample
    int64_t total = 0;      // index of the next sample
    bool started = false;   // a process call has been accepted
    // sdr_chan_process_host: the upload, through pinned memory (allocated by the first such call)
    void *h_pin = nullptr, *d_in = nullptr;
    hipEvent_t uploaded = nullptr;
    // the IQ correction (launch_chan_iqc while one is set) and the raw stream's sums (iq_sums_dev.h)
    bool corrected = false;
    sdr_iq_correction corr{};
    sdr::IqSums sums;
};

namespace sdr {
const sdr_chan_config &chan_config(const sdr_chan *chan) { return chan->cfg; }  // chain.h
hipStream_t chan_stream(const sdr_chan *chan) { return chan->stream; }
}

namespace {

int check_call(sdr_chan *c, const void *in, size_t n_in, const float *out, size_t stride, bool in_on_device)
{
    if (!c || !in || !out)
        return cfail(SDR_ERR_BAD_ARG, "null channelizer, input or output");
    const size_t D = (size_t)c->cfg.decimation;
    if (n_in == 0 || n_in % D != 0 || n_in > (size_t)c->cfg.max_in_samples)
        return cfail(SDR_ERR_BAD_SIZE, "n_in_samples must be a positive multiple of the decimation, at most max_in_samples");
    if ((in_on_device && ((uintptr_t)in & 15u)) || ((uintptr_t)out & 15u))
        return cfail(SDR_ERR_BAD_ARG, "in_dev and out_dev must be 16-byte aligned");
    if (stride % 4 != 0 || stride < n_in / D)
        return cfail(SDR_ERR_BAD_ARG, "band_stride_samples must be a multiple of 4 and at least the outputs per channel");
    return SDR_OK;
}

int run(sdr_chan *c, const void *in_dev, size_t n_in, float *out_dev, size_t stride)
{
    const sdr_chan_config &g = c->cfg;
    sdr::ChanLaunch l{};
    l.fmt = g.in_format;
    l.in = in_dev;
    l.carry = c->d_carry[c->cur];
    l.nco = c->d_nco;
    l.taps = c->d_taps;
    l.channels = c->d_channels;
    l.out = out_dev;
    l.out_stride = stride;
    l.first = c->total;
    l.origin = c->origin;
    l.n_in = (int)n_in;
    l.n_out = g.n_out;
    l.n_channels = g.n_channels;
    l.decimation = g.decimation;
    l.n_taps = g.n_taps;
    CHIP(c->corrected ? sdr::launch_chan_iqc(l, c->corr, c->stream) : sdr::launch_chan(l, c->stream));
    CHIP(sdr::launch_ddc_carry(g.in_format, c->d_carry[c->cur], in_dev, (int)n_in, g.n_taps, c->d_carry[1 - c->cur], c->stream));
    if (c->sums.on)
        CHIP(sdr::iq_sums_add(c->sums, g.in_format, in_dev, (int)n_in, c->stream));
    c->cur = 1 - c->cur;
    c->total += (int64_t)n_in;
    c->started = true;
    return SDR_OK;
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int sdr_chan_tile_outputs(int n_channels, int decimation, int n_taps)
{
    const sdr::ChanShape s = sdr::chan_shape(n_channels, decimation, n_taps);
    return s.log_m < 0 ? -SDR_ERR_BAD_ARG : s.tile;  // (a count, not a status: no error text is set)
}

int sdr_chan_destroy(sdr_chan *c)
{
    if (!c)
        return SDR_OK;
    (void)hipSetDevice(c->cfg.device_id);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(c->d_taps);
    (void)hipFree(c->d_nco);
    (void)hipFree(c->d_channels);
    (void)hipFree(c->d_carry[0]);
    (void)hipFree(c->d_carry[1]);
    (void)hipFree(c->d_in);
    sdr::iq_sums_free(c->sums);
    if (c->h_pin)
        (void)hipHostFree(c->h_pin);
    if (c->uploaded)
        (void)hipEventDestroy(c->uploaded);
    delete c;
    return SDR_OK;
}

int sdr_chan_create(const sdr_chan_config *cfg, const float *taps, const int32_t *channels, sdr_chan **out)
{
    if (!cfg || !taps || !out)
        return cfail(SDR_ERR_BAD_ARG, "null config, taps or output");
    if (cfg->struct_size != (int32_t)sizeof(sdr_chan_config))
        return cfail(SDR_ERR_BAD_ARG, "sdr_chan_config.struct_size mismatch");
    if (sdr::chan_log_m(cfg->n_channels, cfg->decimation, cfg->n_taps) < 0)
        return cfail(SDR_ERR_BAD_ARG, "n_channels must be a power of two in 2 .. 256, decimation n_channels, n_channels / 2 or "
                                      "n_channels / 4 (at least 1), n_taps a multiple of n_channels, 1 .. 64 times it and at most 4096");
    if (!sdr::ddc_format_valid(cfg->in_format))
        return cfail(SDR_ERR_BAD_ARG, "in_format must be SDR_DDC_F32, _SC16, _CS8, _CU8 or SDR_DDC_RF32, _RS16, _RS8, _RU8");
    if (cfg->max_in_samples < cfg->decimation || cfg->max_in_samples % cfg->decimation != 0)
        return cfail(SDR_ERR_BAD_ARG, "max_in_samples must be a positive multiple of the decimation");
    if (cfg->n_out < 1 || cfg->n_out > cfg->n_channels)
        return cfail(SDR_ERR_BAD_ARG, "n_out must be 1 .. n_channels");
    std::vector<int> list((size_t)cfg->n_out);
    std::vector<char> seen((size_t)cfg->n_channels, 0);
    for (int i = 0; i < cfg->n_out; i++) {
        const int ch = channels ? channels[i] : i;
        if (ch < 0 || ch >= cfg->n_channels || seen[(size_t)ch])
            return cfail(SDR_ERR_BAD_ARG, "the channels must be distinct and lie in 0 .. n_channels - 1");
        seen[(size_t)ch] = 1;
        list[(size_t)i] = ch;
    }
    CHIP(hipSetDevice(cfg->device_id));
    sdr_chan *c = new sdr_chan();
    c->cfg = *cfg;
    // (a failure half way frees what was allocated so far: sdr_chan_destroy tolerates null members)
#define CCREATE(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            const std::string _msg = std::string(#expr) + ": " + hipGetErrorString(_e);     \
            sdr_chan_destroy(c);                                                            \
            return cfail(SDR_ERR_HIP, _msg);                                                \
        }                                                                                   \
    } while (0)
    const size_t T = (size_t)cfg->n_taps, keep = T > 1 ? T - 1 : 1;
    CCREATE(hipMalloc((void **)&c->d_taps, sizeof(float) * T));
    CCREATE(hipMalloc((void **)&c->d_nco, sizeof(float2) * (size_t)SDR_DDC_NCO_SIZE));
    CCREATE(hipMalloc((void **)&c->d_channels, sizeof(int) * list.size()));
    for (int i = 0; i < 2; i++) {
        CCREATE(hipMalloc(&c->d_carry[i], sample_bytes(cfg->in_format) * keep));
        CCREATE(hipMemset(c->d_carry[i], 0, sample_bytes(cfg->in_format) * keep));
    }
    std::vector<float> co((size_t)SDR_DDC_NCO_SIZE), si((size_t)SDR_DDC_NCO_SIZE);
    sdr::build_nco(co.data(), si.data());
    std::vector<float2> tab((size_t)SDR_DDC_NCO_SIZE);
    for (size_t i = 0; i < tab.size(); i++)
        tab[i] = make_float2(co[i], si[i]);
    CCREATE(hipMemcpy(c->d_nco, tab.data(), sizeof(float2) * tab.size(), hipMemcpyHostToDevice));
    CCREATE(hipMemcpy(c->d_taps, taps, sizeof(float) * T, hipMemcpyHostToDevice));
    CCREATE(hipMemcpy(c->d_channels, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice));
#undef CCREATE
    *out = c;
    return SDR_OK;
}

int sdr_chan_sync(sdr_chan *c)
{
    if (!c)
        return cfail(SDR_ERR_BAD_ARG, "null channelizer");
    CHIP(hipSetDevice(c->cfg.device_id));
    CHIP(hipStreamSynchronize(c->stream));
    return SDR_OK;
}

int sdr_chan_set_stream(sdr_chan *c, void *hip_stream)
{
    if (!c)
        return cfail(SDR_ERR_BAD_ARG, "null channelizer");
    CHIP(hipSetDevice(c->cfg.device_id));
    CHIP(hipStreamSynchronize(c->stream));  // (the carry of the calls so far is ordered by the old stream)
    c->stream = (hipStream_t)hip_stream;
    return SDR_OK;
}

int sdr_chan_set_first_sample(sdr_chan *c, int64_t k0)
{
    if (!c)
        return cfail(SDR_ERR_BAD_ARG, "null channelizer");
    if (c->started)
        return cfail(SDR_ERR_STATE, "sdr_chan_set_first_sample: the channelizer has processed samples (call it right after sdr_chan_create)");
    if (k0 < 0 || k0 % c->cfg.decimation != 0)
        return cfail(SDR_ERR_BAD_ARG, "the first sample must be >= 0 and a multiple of the decimation");
    c->origin = c->total = k0;
    return SDR_OK;
}

int64_t sdr_chan_total_samples(sdr_chan *c) { return c ? c->total : 0; }

int sdr_chan_process_device(sdr_chan *c, const void *in_dev, size_t n_in_samples, float *out_dev, size_t band_stride_samples)
{
    const int rc = check_call(c, in_dev, n_in_samples, out_dev, band_stride_samples, true);
    if (rc)
        return rc;
    CHIP(hipSetDevice(c->cfg.device_id));
    return run(c, in_dev, n_in_samples, out_dev, band_stride_samples);
}

int sdr_chan_process_host(sdr_chan *c, const void *in_host, size_t n_in_samples, float *out_dev, size_t band_stride_samples)
{
    const int rc = check_call(c, in_host, n_in_samples, out_dev, band_stride_samples, false);
    if (rc)
        return rc;
    CHIP(hipSetDevice(c->cfg.device_id));
    const size_t cap = sample_bytes(c->cfg.in_format) * (size_t)c->cfg.max_in_samples;
    if (!c->d_in)
        CHIP(hipMalloc(&c->d_in, cap));
    if (!c->h_pin)
        CHIP(hipHostMalloc(&c->h_pin, cap, hipHostMallocDefault));
    if (!c->uploaded)
        CHIP(hipEventCreateWithFlags(&c->uploaded, hipEventDisableTiming));
    else
        CHIP(hipEventSynchronize(c->uploaded));  // the pinned buffer is free once the last upload has left it
    const size_t bytes = sample_bytes(c->cfg.in_format) * n_in_samples;
    memcpy(c->h_pin, in_host, bytes);
    CHIP(hipMemcpyAsync(c->d_in, c->h_pin, bytes, hipMemcpyHostToDevice, c->stream));
    CHIP(hipEventRecord(c->uploaded, c->stream));
    return run(c, c->d_in, n_in_samples, out_dev, band_stride_samples);
}

int sdr_iq_chan_set_correction(sdr_chan *c, const sdr_iq_correction *v)
{
    if (!c)
        return cfail(SDR_ERR_BAD_ARG, "null channelizer");
    if (sdr::ddc_is_real(c->cfg.in_format))
        return cfail(SDR_ERR_BAD_ARG, "sdr_iq_chan_set_correction: a real input format has no IQ correction");
    if (v && !(std::isfinite(v->dc_re) && std::isfinite(v->dc_im) && std::isfinite(v->gain_im) && std::isfinite(v->cross)))
        return cfail(SDR_ERR_BAD_ARG, "sdr_iq_chan_set_correction: every field must be finite");
    c->corrected = v != nullptr;
    c->corr = v ? *v : sdr_iq_correction{};
    return SDR_OK;
}

int sdr_iq_chan_enable_sums(sdr_chan *c, int on)
{
    if (!c)
        return cfail(SDR_ERR_BAD_ARG, "null channelizer");
    if (!sdr::iq_sums_format(c->cfg.in_format))
        return cfail(SDR_ERR_BAD_ARG, "sdr_iq_chan_enable_sums: sums are offered for SDR_DDC_CS8, _CU8 and _SC16");
    CHIP(hipSetDevice(c->cfg.device_id));
    CHIP(sdr::iq_sums_enable(c->sums, c->cfg.in_format, c->cfg.max_in_samples, on != 0, c->stream));
    return SDR_OK;
}

int sdr_iq_chan_read_sums(sdr_chan *c, sdr_iq_sums *out)
{
    if (!c || !out)
        return cfail(SDR_ERR_BAD_ARG, "null channelizer or output");
    if (!c->sums.on)
        return cfail(SDR_ERR_STATE, "sdr_iq_chan_read_sums: the sums are off (sdr_iq_chan_enable_sums)");
    CHIP(hipSetDevice(c->cfg.device_id));
    CHIP(sdr::iq_sums_read(c->sums, out, c->stream));
    return SDR_OK;
}

#pragma GCC visibility pop
}
