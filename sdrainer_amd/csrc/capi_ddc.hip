// capi_ddc.hip — the down-converter behind the C ABI (include/sdrainer_hip.h "down-converter"): an object of its own beside
// the bank, with the taps, the NCO table and the carry of n_taps - 1 raw samples in device memory.  The kernel is k_ddc.h, instantiated by
// k_ddc.hip (complex formats) and k_ddc_real.hip (real formats); a sample's size is host/ddc_format.h's.
//
// What the object shares with the other front-end objects is front.h's: the stream and the sample clock (FrontObject), the
// double-buffered carry (RawCarry), process_host's upload (HostUpload), the IQ state (IqFront) and the checks of a call.
// Here are the config's validation, the launch descriptor, the steps and every message.  Everything is ordered by the DDC's
// one stream.
//
// While an IQ correction is set (sdr_iq_ddc_set_correction) a call launches k_ddc_iqc.hip's instance in place of k_ddc.hip's;
// with the sums on (iq_sums_dev.h) k_iq_sums.hip's reduction over the call's input follows the carry's kernel.
#include "front.h"

using sdr::fail;

struct sdr_ddc : sdr::FrontObject {
    sdr_ddc_config cfg{};
    sdr::DdcSteps steps{};
    float *d_taps = nullptr;
    float2 *d_nco = nullptr;
    sdr::RawCarry carry;
    sdr::HostUpload upload;  // sdr_ddc_process_host
    sdr::IqFront iq;         // launch_ddc_iqc while a correction is set
};

namespace sdr {
const sdr_ddc_config &ddc_config(const sdr_ddc *ddc) { return ddc->cfg; }  // chain.h
hipStream_t ddc_stream(const sdr_ddc *ddc) { return ddc->stream; }
}

namespace {

size_t sample_bytes(int fmt) { return (size_t)sdr::ddc_sample_bytes(fmt); }  // 8, 4, 2 complex; 4, 2, 1 real

const sdr::CallTexts kCall = {"null ddc, input or output",
                              "n_in_samples must be a positive multiple of the decimation, at most max_in_samples",
                              "in_dev and out_dev must be 16-byte aligned"};
const sdr::IqTexts kIq = {"null ddc",
                          "null ddc or output",
                          "sdr_iq_ddc_set_correction: a real input format has no IQ correction",
                          "sdr_iq_ddc_set_correction: every field must be finite",
                          "sdr_iq_ddc_enable_sums: sums are offered for SDR_DDC_CS8, _CU8 and _SC16",
                          "sdr_iq_ddc_read_sums: the sums are off (sdr_iq_ddc_enable_sums)"};

int check_call(sdr_ddc *d, const void *in, size_t n_in, const float *out, size_t stride, bool in_on_device)
{
    const int rc = sdr::check_call(d, in, n_in, out, in_on_device, kCall);
    if (rc)
        return rc;
    if (!sdr::stride_ok(stride, n_in / (size_t)d->cfg.decimation))
        return fail(SDR_ERR_BAD_ARG, "band_stride_samples must be a multiple of 4 and at least the outputs per band");
    return SDR_OK;
}

int run(sdr_ddc *d, const void *in_dev, size_t n_in, float *out_dev, size_t stride)
{
    const sdr_ddc_config &c = d->cfg;
    sdr::DdcLaunch l{};
    l.fmt = c.in_format;
    l.in = in_dev;
    l.carry = d->carry.cur();
    l.nco = d->d_nco;
    l.taps = d->d_taps;
    l.out = out_dev;
    l.out_stride = stride;
    l.first = d->clock.total;
    l.origin = d->clock.origin;
    l.n_in = (int)n_in;
    l.n_bands = c.n_bands;
    l.decimation = c.decimation;
    l.n_taps = c.n_taps;
    l.steps = d->steps;
    HIP_TRY(d->iq.corrected ? sdr::launch_ddc_iqc(l, d->iq.corr, d->stream) : sdr::launch_ddc(l, d->stream));
    const int rc = d->iq.after_launch(c.in_format, d->carry, in_dev, (int)n_in, c.n_taps, d->stream);
    if (rc)
        return rc;
    d->clock.advance(n_in);
    return SDR_OK;
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int sdr_ddc_nco_table(float *cos_out, float *sin_out)
{
    sdr::build_nco(cos_out, sin_out);
    return SDR_OK;
}

int sdr_ddc_destroy(sdr_ddc *d)
{
    if (!d)
        return SDR_OK;
    d->quiesce();
    (void)hipFree(d->d_taps);
    (void)hipFree(d->d_nco);
    d->carry.release();
    sdr::iq_sums_free(d->iq.sums);
    d->upload.release();
    delete d;
    return SDR_OK;
}

int sdr_ddc_create(const sdr_ddc_config *cfg, const float *taps, const int32_t *nco_steps, sdr_ddc **out)
{
    if (!cfg || !taps || !nco_steps || !out)
        return fail(SDR_ERR_BAD_ARG, "null config, taps, steps or output");
    if (cfg->struct_size != (int32_t)sizeof(sdr_ddc_config))
        return fail(SDR_ERR_BAD_ARG, "sdr_ddc_config.struct_size mismatch");
    if (cfg->n_bands < 1 || cfg->n_bands > sdr::kDdcMaxBands)
        return fail(SDR_ERR_BAD_ARG, "n_bands must be 1 .. 64");
    if (cfg->decimation < 1 || cfg->decimation > sdr::kDdcMaxDecimation)
        return fail(SDR_ERR_BAD_ARG, "decimation must be 1 .. 256");
    if (cfg->n_taps < 1 || cfg->n_taps > sdr::kDdcMaxTaps)
        return fail(SDR_ERR_BAD_ARG, "n_taps must be 1 .. 4096");
    if (!sdr::ddc_format_valid(cfg->in_format))
        return fail(SDR_ERR_BAD_ARG, "in_format must be SDR_DDC_F32, _SC16, _CS8, _CU8 or SDR_DDC_RF32, _RS16, _RS8, _RU8");
    if (cfg->max_in_samples < cfg->decimation || cfg->max_in_samples % cfg->decimation != 0)
        return fail(SDR_ERR_BAD_ARG, "max_in_samples must be a positive multiple of the decimation");
    if (cfg->reserved != 0)
        return fail(SDR_ERR_BAD_ARG, "sdr_ddc_config.reserved must be 0");
    for (int b = 0; b < cfg->n_bands; b++)
        if (!sdr::step_valid(nco_steps[b]))
            return fail(SDR_ERR_BAD_ARG, "an NCO step must lie in [-32768, 32767]");
    HIP_TRY(hipSetDevice(cfg->device_id));
    sdr::Building<sdr_ddc, sdr_ddc_destroy> d(new sdr_ddc());
    d->cfg = *cfg;
    d->place(cfg->device_id, cfg->decimation, cfg->max_in_samples);
    for (int b = 0; b < cfg->n_bands; b++)
        d->steps.step[b] = (int16_t)nco_steps[b];
    HIP_TRY(hipMalloc((void **)&d->d_taps, sizeof(float) * (size_t)cfg->n_taps));
    HIP_TRY(hipMalloc((void **)&d->d_nco, sizeof(float2) * (size_t)sdr::kDdcNco));
    int rc = d->carry.alloc(sample_bytes(cfg->in_format) * sdr::carry_samples(cfg->n_taps));
    if (rc || (rc = sdr::upload_coefficients(d->d_taps, d->d_nco, taps, cfg->n_taps)))
        return rc;
    *out = d.release();
    return SDR_OK;
}

int sdr_ddc_sync(sdr_ddc *d) { return sdr::front_sync(d, "null ddc"); }

int sdr_ddc_set_stream(sdr_ddc *d, void *hip_stream) { return sdr::front_set_stream(d, hip_stream, "null ddc"); }

int sdr_ddc_set_first_sample(sdr_ddc *d, int64_t k0)
{
    return sdr::front_set_first_sample(d, k0, "null ddc",
                                       "sdr_ddc_set_first_sample: the DDC has processed samples (call it right after sdr_ddc_create)",
                                       "the first sample must be >= 0 and a multiple of the decimation");
}

int64_t sdr_ddc_total_samples(sdr_ddc *d) { return sdr::front_total_samples(d); }

int sdr_ddc_set_nco_step(sdr_ddc *d, int band, int step)
{
    if (!d)
        return fail(SDR_ERR_BAD_ARG, "null ddc");
    if (band < 0 || band >= d->cfg.n_bands)
        return fail(SDR_ERR_BAD_ARG, "band out of range");
    if (!sdr::step_valid(step))
        return fail(SDR_ERR_BAD_ARG, "an NCO step must lie in [-32768, 32767]");
    d->steps.step[band] = (int16_t)step;
    return SDR_OK;
}

int sdr_ddc_process_device(sdr_ddc *d, const void *in_dev, size_t n_in_samples, float *out_dev, size_t band_stride_samples)
{
    const int rc = check_call(d, in_dev, n_in_samples, out_dev, band_stride_samples, true);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(d->device_id));
    return run(d, in_dev, n_in_samples, out_dev, band_stride_samples);
}

int sdr_ddc_process_host(sdr_ddc *d, const void *in_host, size_t n_in_samples, float *out_dev, size_t band_stride_samples)
{
    int rc = check_call(d, in_host, n_in_samples, out_dev, band_stride_samples, false);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(d->device_id));
    const size_t sb = sample_bytes(d->cfg.in_format);
    if ((rc = d->upload.stage(in_host, sb * n_in_samples, sb * (size_t)d->cfg.max_in_samples, nullptr, d->stream)))
        return rc;
    return run(d, d->upload.d_in, n_in_samples, out_dev, band_stride_samples);
}

int sdr_iq_ddc_set_correction(sdr_ddc *d, const sdr_iq_correction *c) { return sdr::iq_set_correction(d, c, kIq); }

int sdr_iq_ddc_enable_sums(sdr_ddc *d, int on) { return sdr::iq_enable_sums(d, on, kIq); }

int sdr_iq_ddc_read_sums(sdr_ddc *d, sdr_iq_sums *out) { return sdr::iq_read_sums(d, out, kIq); }

int sdr_iq_correction_from_sums(const sdr_iq_sums *s, int in_format, sdr_iq_correction *out)
{
    if (!s || !out)
        return fail(SDR_ERR_BAD_ARG, "null sums or output");
    if (!sdr::iq_correction_from_sums(*s, in_format, out))
        return fail(SDR_ERR_BAD_ARG, "sdr_iq_correction_from_sums: a format without sums, n < 2, no variance of I, a Q that is a "
                                     "multiple of I, or a value that is not finite");
    return SDR_OK;
}

#pragma GCC visibility pop
}
