// capi_chan.hip — the polyphase channelizer behind the C ABI (include/sdrainer_hip.h "channelizer"): an object of its own
// beside the bank and the down-converter, with the taps, the table of twiddles, the channel list and the carry of n_taps - 1
// raw samples in device memory.  The kernel is k_chan.h, instantiated by k_chan.hip; a sample's size is host/ddc_format.h's.
//
// The stream and the sample clock, the carry (formed by launch_ddc_carry behind each call's kernel), process_host's upload,
// the IQ state and the checks of a call are front.h's, shared with the down-converter: k_chan_iqc.hip's instance runs while
// a correction is set, k_iq_sums.hip behind the carry's kernel with the sums on.  Here are the config's validation, the
// launch descriptor and every message.  Everything is ordered by the channelizer's one stream.
#include "chan.h"
#include "front.h"

using sdr::fail;

struct sdr_chan : sdr::FrontObject {
    sdr_chan_config cfg{};
    float *d_taps = nullptr;
    float2 *d_nco = nullptr;
    int *d_channels = nullptr;
    sdr::RawCarry carry;
    sdr::HostUpload upload;  // sdr_chan_process_host
    sdr::IqFront iq;         // launch_chan_iqc while a correction is set
};

namespace sdr {
const sdr_chan_config &chan_config(const sdr_chan *chan) { return chan->cfg; }  // chain.h
hipStream_t chan_stream(const sdr_chan *chan) { return chan->stream; }
}

namespace {

size_t sample_bytes(int fmt) { return (size_t)sdr::ddc_sample_bytes(fmt); }  // 8, 4, 2 complex; 4, 2, 1 real

const sdr::CallTexts kCall = {"null channelizer, input or output",
                              "n_in_samples must be a positive multiple of the decimation, at most max_in_samples",
                              "in_dev and out_dev must be 16-byte aligned"};
const sdr::IqTexts kIq = {"null channelizer",
                          "null channelizer or output",
                          "sdr_iq_chan_set_correction: a real input format has no IQ correction",
                          "sdr_iq_chan_set_correction: every field must be finite",
                          "sdr_iq_chan_enable_sums: sums are offered for SDR_DDC_CS8, _CU8 and _SC16",
                          "sdr_iq_chan_read_sums: the sums are off (sdr_iq_chan_enable_sums)"};

int check_call(sdr_chan *c, const void *in, size_t n_in, const float *out, size_t stride, bool in_on_device)
{
    const int rc = sdr::check_call(c, in, n_in, out, in_on_device, kCall);
    if (rc)
        return rc;
    if (!sdr::stride_ok(stride, n_in / (size_t)c->cfg.decimation))
        return fail(SDR_ERR_BAD_ARG, "band_stride_samples must be a multiple of 4 and at least the outputs per channel");
    return SDR_OK;
}

int run(sdr_chan *c, const void *in_dev, size_t n_in, float *out_dev, size_t stride)
{
    const sdr_chan_config &g = c->cfg;
    sdr::ChanLaunch l{};
    l.fmt = g.in_format;
    l.in = in_dev;
    l.carry = c->carry.cur();
    l.nco = c->d_nco;
    l.taps = c->d_taps;
    l.channels = c->d_channels;
    l.out = out_dev;
    l.out_stride = stride;
    l.first = c->clock.total;
    l.origin = c->clock.origin;
    l.n_in = (int)n_in;
    l.n_out = g.n_out;
    l.n_channels = g.n_channels;
    l.decimation = g.decimation;
    l.n_taps = g.n_taps;
    HIP_TRY(c->iq.corrected ? sdr::launch_chan_iqc(l, c->iq.corr, c->stream) : sdr::launch_chan(l, c->stream));
    const int rc = c->iq.after_launch(g.in_format, c->carry, in_dev, (int)n_in, g.n_taps, c->stream);
    if (rc)
        return rc;
    c->clock.advance(n_in);
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
    c->quiesce();
    (void)hipFree(c->d_taps);
    (void)hipFree(c->d_nco);
    (void)hipFree(c->d_channels);
    c->carry.release();
    sdr::iq_sums_free(c->iq.sums);
    c->upload.release();
    delete c;
    return SDR_OK;
}

int sdr_chan_create(const sdr_chan_config *cfg, const float *taps, const int32_t *channels, sdr_chan **out)
{
    if (!cfg || !taps || !out)
        return fail(SDR_ERR_BAD_ARG, "null config, taps or output");
    if (cfg->struct_size != (int32_t)sizeof(sdr_chan_config))
        return fail(SDR_ERR_BAD_ARG, "sdr_chan_config.struct_size mismatch");
    if (sdr::chan_log_m(cfg->n_channels, cfg->decimation, cfg->n_taps) < 0)
        return fail(SDR_ERR_BAD_ARG, "n_channels must be a power of two in 2 .. 256, decimation n_channels, n_channels / 2 or "
                                     "n_channels / 4 (at least 1), n_taps a multiple of n_channels, 1 .. 64 times it and at most 4096");
    if (!sdr::ddc_format_valid(cfg->in_format))
        return fail(SDR_ERR_BAD_ARG, "in_format must be SDR_DDC_F32, _SC16, _CS8, _CU8 or SDR_DDC_RF32, _RS16, _RS8, _RU8");
    if (cfg->max_in_samples < cfg->decimation || cfg->max_in_samples % cfg->decimation != 0)
        return fail(SDR_ERR_BAD_ARG, "max_in_samples must be a positive multiple of the decimation");
    if (cfg->n_out < 1 || cfg->n_out > cfg->n_channels)
        return fail(SDR_ERR_BAD_ARG, "n_out must be 1 .. n_channels");
    std::vector<int> list((size_t)cfg->n_out);
    std::vector<char> seen((size_t)cfg->n_channels, 0);
    for (int i = 0; i < cfg->n_out; i++) {
        const int ch = channels ? channels[i] : i;
        if (ch < 0 || ch >= cfg->n_channels || seen[(size_t)ch])
            return fail(SDR_ERR_BAD_ARG, "the channels must be distinct and lie in 0 .. n_channels - 1");
        seen[(size_t)ch] = 1;
        list[(size_t)i] = ch;
    }
    HIP_TRY(hipSetDevice(cfg->device_id));
    sdr::Building<sdr_chan, sdr_chan_destroy> c(new sdr_chan());
    c->cfg = *cfg;
    c->place(cfg->device_id, cfg->decimation, cfg->max_in_samples);
    HIP_TRY(hipMalloc((void **)&c->d_taps, sizeof(float) * (size_t)cfg->n_taps));
    HIP_TRY(hipMalloc((void **)&c->d_nco, sizeof(float2) * (size_t)sdr::kDdcNco));
    HIP_TRY(hipMalloc((void **)&c->d_channels, sizeof(int) * list.size()));
    int rc = c->carry.alloc(sample_bytes(cfg->in_format) * sdr::carry_samples(cfg->n_taps));
    if (rc || (rc = sdr::upload_coefficients(c->d_taps, c->d_nco, taps, cfg->n_taps)))
        return rc;
    HIP_TRY(hipMemcpy(c->d_channels, list.data(), sizeof(int) * list.size(), hipMemcpyHostToDevice));
    *out = c.release();
    return SDR_OK;
}

int sdr_chan_sync(sdr_chan *c) { return sdr::front_sync(c, "null channelizer"); }

int sdr_chan_set_stream(sdr_chan *c, void *hip_stream) { return sdr::front_set_stream(c, hip_stream, "null channelizer"); }

int sdr_chan_set_first_sample(sdr_chan *c, int64_t k0)
{
    return sdr::front_set_first_sample(c, k0, "null channelizer",
                                       "sdr_chan_set_first_sample: the channelizer has processed samples (call it right after sdr_chan_create)",
                                       "the first sample must be >= 0 and a multiple of the decimation");
}

int64_t sdr_chan_total_samples(sdr_chan *c) { return sdr::front_total_samples(c); }

int sdr_chan_process_device(sdr_chan *c, const void *in_dev, size_t n_in_samples, float *out_dev, size_t band_stride_samples)
{
    const int rc = check_call(c, in_dev, n_in_samples, out_dev, band_stride_samples, true);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(c->device_id));
    return run(c, in_dev, n_in_samples, out_dev, band_stride_samples);
}

int sdr_chan_process_host(sdr_chan *c, const void *in_host, size_t n_in_samples, float *out_dev, size_t band_stride_samples)
{
    int rc = check_call(c, in_host, n_in_samples, out_dev, band_stride_samples, false);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(c->device_id));
    const size_t sb = sample_bytes(c->cfg.in_format);
    if ((rc = c->upload.stage(in_host, sb * n_in_samples, sb * (size_t)c->cfg.max_in_samples, nullptr, c->stream)))
        return rc;
    return run(c, c->upload.d_in, n_in_samples, out_dev, band_stride_samples);
}

int sdr_iq_chan_set_correction(sdr_chan *c, const sdr_iq_correction *v) { return sdr::iq_set_correction(c, v, kIq); }

int sdr_iq_chan_enable_sums(sdr_chan *c, int on) { return sdr::iq_enable_sums(c, on, kIq); }

int sdr_iq_chan_read_sums(sdr_chan *c, sdr_iq_sums *out) { return sdr::iq_read_sums(c, out, kIq); }

#pragma GCC visibility pop
}
