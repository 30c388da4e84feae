// capi_ddc.hip — the down-converter behind the C ABI (include/sdrainer_hip.h "down-converter"): an object of its own beside
// the bank, with the taps, the NCO table and the carry of n_taps - 1 raw samples in device memory.  The kernel is k_ddc.h, instantiated by
// k_ddc.hip (complex formats) and k_ddc_real.hip (real formats); a sample's size is host/ddc_format.h's.
//
// The carry is double-buffered: a call's kernel reads carry[cur] and a second small kernel behind it forms carry[1 - cur]
// from carry[cur] and the call's input - also where the call is shorter than n_taps - 1 samples and part of the old carry
// survives.  Everything is ordered by the DDC's one stream.
//
// While an IQ correction is set (sdr_iq_ddc_set_correction) a call launches k_ddc_iqc.hip's instance in place of k_ddc.hip's;
// with the sums on (iq_sums_dev.h) k_iq_sums.hip's reduction over the call's input follows the carry's kernel.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ddc.h"
#include "host/ddc_format.h"
#include "iq_sums_dev.h"
#include "host/nco_table.h"

namespace sdr {
int set_error(int code, const char *msg);  // capi_bank.hip: feeds sdr_last_error()
}

namespace {

int dfail(int code, const std::string &msg) { return sdr::set_error(code, msg.c_str()); }
#define DHIP(expr)                                                                          \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return dfail(SDR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

size_t sample_bytes(int fmt) { return (size_t)sdr::ddc_sample_bytes(fmt); }  // 8, 4, 2 complex; 4, 2, 1 real

using sdr::build_nco;  // host/nco_table.h: the channelizer builds the same table

}  // namespace

struct sdr_ddc {
    sdr_ddc_config cfg{};
    hipStream_t stream = nullptr;
    sdr::DdcSteps steps{};
    float *d_taps = nullptr;
    float2 *d_nco = nullptr;
    void *d_carry[2] = {nullptr, nullptr};
    int cur = 0;            // the carry buffer the next call reads
    int64_t origin = 0;     // index of the DDC's first sample
    int64_t total = 0;      // index of the next sample
    bool started = false;   // a process call has been accepted
    // sdr_ddc_process_host: the upload, through pinned memory (allocated by the first such call)
    void *h_pin = nullptr, *d_in = nullptr;
    hipEvent_t uploaded = nullptr;
    // the IQ correction (launch_ddc_iqc while one is set) and the raw stream's sums (iq_sums_dev.h)
    bool corrected = false;
    sdr_iq_correction corr{};
    sdr::IqSums sums;
};

namespace sdr {
const sdr_ddc_config &ddc_config(const sdr_ddc *ddc) { return ddc->cfg; }  // chain.h
hipStream_t ddc_stream(const sdr_ddc *ddc) { return ddc->stream; }
}

namespace {

int check_call(sdr_ddc *d, const void *in, size_t n_in, const float *out, size_t stride, bool in_on_device)
{
    if (!d || !in || !out)
        return dfail(SDR_ERR_BAD_ARG, "null ddc, input or output");
    const size_t D = (size_t)d->cfg.decimation;
    if (n_in == 0 || n_in % D != 0 || n_in > (size_t)d->cfg.max_in_samples)
        return dfail(SDR_ERR_BAD_SIZE, "n_in_samples must be a positive multiple of the decimation, at most max_in_samples");
    if ((in_on_device && ((uintptr_t)in & 15u)) || ((uintptr_t)out & 15u))
        return dfail(SDR_ERR_BAD_ARG, "in_dev and out_dev must be 16-byte aligned");
    if (stride % 4 != 0 || stride < n_in / D)
        return dfail(SDR_ERR_BAD_ARG, "band_stride_samples must be a multiple of 4 and at least the outputs per band");
    return SDR_OK;
}

int run(sdr_ddc *d, const void *in_dev, size_t n_in, float *out_dev, size_t stride)
{
    const sdr_ddc_config &c = d->cfg;
    sdr::DdcLaunch l{};
    l.fmt = c.in_format;
    l.in = in_dev;
    l.carry = d->d_carry[d->cur];
    l.nco = d->d_nco;
    l.taps = d->d_taps;
    l.out = out_dev;
    l.out_stride = stride;
    l.first = d->total;
    l.origin = d->origin;
    l.n_in = (int)n_in;
    l.n_bands = c.n_bands;
    l.decimation = c.decimation;
    l.n_taps = c.n_taps;
    l.steps = d->steps;
    DHIP(d->corrected ? sdr::launch_ddc_iqc(l, d->corr, d->stream) : sdr::launch_ddc(l, d->stream));
    DHIP(sdr::launch_ddc_carry(c.in_format, d->d_carry[d->cur], in_dev, (int)n_in, c.n_taps, d->d_carry[1 - d->cur], d->stream));
    if (d->sums.on)
        DHIP(sdr::iq_sums_add(d->sums, c.in_format, in_dev, (int)n_in, d->stream));
    d->cur = 1 - d->cur;
    d->total += (int64_t)n_in;
    d->started = true;
    return SDR_OK;
}

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int sdr_ddc_nco_table(float *cos_out, float *sin_out)
{
    build_nco(cos_out, sin_out);
    return SDR_OK;
}

int sdr_ddc_destroy(sdr_ddc *d)
{
    if (!d)
        return SDR_OK;
    (void)hipSetDevice(d->cfg.device_id);
    (void)hipStreamSynchronize(d->stream);
    (void)hipFree(d->d_taps);
    (void)hipFree(d->d_nco);
    (void)hipFree(d->d_carry[0]);
    (void)hipFree(d->d_carry[1]);
    (void)hipFree(d->d_in);
    sdr::iq_sums_free(d->sums);
    if (d->h_pin)
        (void)hipHostFree(d->h_pin);
    if (d->uploaded)
        (void)hipEventDestroy(d->uploaded);
    delete d;
    return SDR_OK;
}

int sdr_ddc_create(const sdr_ddc_config *cfg, const float *taps, const int32_t *nco_steps, sdr_ddc **out)
{
    if (!cfg || !taps || !nco_steps || !out)
        return dfail(SDR_ERR_BAD_ARG, "null config, taps, steps or output");
    if (cfg->struct_size != (int32_t)sizeof(sdr_ddc_config))
        return dfail(SDR_ERR_BAD_ARG, "sdr_ddc_config.struct_size mismatch");
    if (cfg->n_bands < 1 || cfg->n_bands > sdr::kDdcMaxBands)
        return dfail(SDR_ERR_BAD_ARG, "n_bands must be 1 .. 64");
    if (cfg->decimation < 1 || cfg->decimation > sdr::kDdcMaxDecimation)
        return dfail(SDR_ERR_BAD_ARG, "decimation must be 1 .. 256");
    if (cfg->n_taps < 1 || cfg->n_taps > sdr::kDdcMaxTaps)
        return dfail(SDR_ERR_BAD_ARG, "n_taps must be 1 .. 4096");
    if (!sdr::ddc_format_valid(cfg->in_format))
        return dfail(SDR_ERR_BAD_ARG, "in_format must be SDR_DDC_F32, _SC16, _CS8, _CU8 or SDR_DDC_RF32, _RS16, _RS8, _RU8");
    if (cfg->max_in_samples < cfg->decimation || cfg->max_in_samples % cfg->decimation != 0)
        return dfail(SDR_ERR_BAD_ARG, "max_in_samples must be a positive multiple of the decimation");
    if (cfg->reserved != 0)
        return dfail(SDR_ERR_BAD_ARG, "sdr_ddc_config.reserved must be 0");
    for (int b = 0; b < cfg->n_bands; b++)
        if (nco_steps[b] < -32768 || nco_steps[b] > 32767)
            return dfail(SDR_ERR_BAD_ARG, "an NCO step must lie in [-32768, 32767]");
    DHIP(hipSetDevice(cfg->device_id));
    sdr_ddc *d = new sdr_ddc();
    d->cfg = *cfg;
    for (int b = 0; b < cfg->n_bands; b++)
        d->steps.step[b] = (int16_t)nco_steps[b];
    // (a failure half way frees what was allocated so far: sdr_ddc_destroy tolerates null members)
#define DCREATE(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            const std::string _msg = std::string(#expr) + ": " + hipGetErrorString(_e);     \
            sdr_ddc_destroy(d);                                                             \
            return dfail(SDR_ERR_HIP, _msg);                                                \
        }                                                                                   \
    } while (0)
    const size_t T = (size_t)cfg->n_taps, keep = T > 1 ? T - 1 : 1;
    DCREATE(hipMalloc((void **)&d->d_taps, sizeof(float) * T));
    DCREATE(hipMalloc((void **)&d->d_nco, sizeof(float2) * (size_t)sdr::kDdcNco));
    for (int i = 0; i < 2; i++) {
        DCREATE(hipMalloc(&d->d_carry[i], sample_bytes(cfg->in_format) * keep));
        DCREATE(hipMemset(d->d_carry[i], 0, sample_bytes(cfg->in_format) * keep));
    }
    std::vector<float> co((size_t)sdr::kDdcNco), si((size_t)sdr::kDdcNco);
    build_nco(co.data(), si.data());
    std::vector<float2> tab((size_t)sdr::kDdcNco);
    for (size_t i = 0; i < tab.size(); i++)
        tab[i] = make_float2(co[i], si[i]);
    DCREATE(hipMemcpy(d->d_nco, tab.data(), sizeof(float2) * tab.size(), hipMemcpyHostToDevice));
    DCREATE(hipMemcpy(d->d_taps, taps, sizeof(float) * T, hipMemcpyHostToDevice));
#undef DCREATE
    *out = d;
    return SDR_OK;
}

int sdr_ddc_sync(sdr_ddc *d)
{
    if (!d)
        return dfail(SDR_ERR_BAD_ARG, "null ddc");
    DHIP(hipSetDevice(d->cfg.device_id));
    DHIP(hipStreamSynchronize(d->stream));
    return SDR_OK;
}

int sdr_ddc_set_stream(sdr_ddc *d, void *hip_stream)
{
    if (!d)
        return dfail(SDR_ERR_BAD_ARG, "null ddc");
    DHIP(hipSetDevice(d->cfg.device_id));
    DHIP(hipStreamSynchronize(d->stream));  // (the carry of the calls so far is ordered by the old stream)
    d->stream = (hipStream_t)hip_stream;
    return SDR_OK;
}

int sdr_ddc_set_first_sample(sdr_ddc *d, int64_t k0)
{
    if (!d)
        return dfail(SDR_ERR_BAD_ARG, "null ddc");
    if (d->started)
        return dfail(SDR_ERR_STATE, "sdr_ddc_set_first_sample: the DDC has processed samples (call it right after sdr_ddc_create)");
    if (k0 < 0 || k0 % d->cfg.decimation != 0)
        return dfail(SDR_ERR_BAD_ARG, "the first sample must be >= 0 and a multiple of the decimation");
    d->origin = d->total = k0;
    return SDR_OK;
}

int64_t sdr_ddc_total_samples(sdr_ddc *d) { return d ? d->total : 0; }

int sdr_ddc_set_nco_step(sdr_ddc *d, int band, int step)
{
    if (!d)
        return dfail(SDR_ERR_BAD_ARG, "null ddc");
    if (band < 0 || band >= d->cfg.n_bands)
        return dfail(SDR_ERR_BAD_ARG, "band out of range");
    if (step < -32768 || step > 32767)
        return dfail(SDR_ERR_BAD_ARG, "an NCO step must lie in [-32768, 32767]");
    d->steps.step[band] = (int16_t)step;
    return SDR_OK;
}

int sdr_ddc_process_device(sdr_ddc *d, const void *in_dev, size_t n_in_samples, float *out_dev, size_t band_stride_samples)
{
    const int rc = check_call(d, in_dev, n_in_samples, out_dev, band_stride_samples, true);
    if (rc)
        return rc;
    DHIP(hipSetDevice(d->cfg.device_id));
    return run(d, in_dev, n_in_samples, out_dev, band_stride_samples);
}

int sdr_ddc_process_host(sdr_ddc *d, const void *in_host, size_t n_in_samples, float *out_dev, size_t band_stride_samples)
{
    const int rc = check_call(d, in_host, n_in_samples, out_dev, band_stride_samples, false);
    if (rc)
        return rc;
    DHIP(hipSetDevice(d->cfg.device_id));
    const size_t cap = sample_bytes(d->cfg.in_format) * (size_t)d->cfg.max_in_samples;
    if (!d->d_in)
        DHIP(hipMalloc(&d->d_in, cap));
    if (!d->h_pin)
        DHIP(hipHostMalloc(&d->h_pin, cap, hipHostMallocDefault));
    if (!d->uploaded)
        DHIP(hipEventCreateWithFlags(&d->uploaded, hipEventDisableTiming));
    else
        DHIP(hipEventSynchronize(d->uploaded));  // the pinned buffer is free once the last upload has left it
    const size_t bytes = sample_bytes(d->cfg.in_format) * n_in_samples;
    memcpy(d->h_pin, in_host, bytes);
    DHIP(hipMemcpyAsync(d->d_in, d->h_pin, bytes, hipMemcpyHostToDevice, d->stream));
    DHIP(hipEventRecord(d->uploaded, d->stream));
    return run(d, d->d_in, n_in_samples, out_dev, band_stride_samples);
}

int sdr_iq_ddc_set_correction(sdr_ddc *d, const sdr_iq_correction *c)
{
    if (!d)
        return dfail(SDR_ERR_BAD_ARG, "null ddc");
    if (sdr::ddc_is_real(d->cfg.in_format))
        return dfail(SDR_ERR_BAD_ARG, "sdr_iq_ddc_set_correction: a real input format has no IQ correction");
    if (c && !(std::isfinite(c->dc_re) && std::isfinite(c->dc_im) && std::isfinite(c->gain_im) && std::isfinite(c->cross)))
        return dfail(SDR_ERR_BAD_ARG, "sdr_iq_ddc_set_correction: every field must be finite");
    d->corrected = c != nullptr;
    d->corr = c ? *c : sdr_iq_correction{};
    return SDR_OK;
}

int sdr_iq_ddc_enable_sums(sdr_ddc *d, int on)
{
    if (!d)
        return dfail(SDR_ERR_BAD_ARG, "null ddc");
    if (!sdr::iq_sums_format(d->cfg.in_format))
        return dfail(SDR_ERR_BAD_ARG, "sdr_iq_ddc_enable_sums: sums are offered for SDR_DDC_CS8, _CU8 and _SC16");
    DHIP(hipSetDevice(d->cfg.device_id));
    DHIP(sdr::iq_sums_enable(d->sums, d->cfg.in_format, d->cfg.max_in_samples, on != 0, d->stream));
    return SDR_OK;
}

int sdr_iq_ddc_read_sums(sdr_ddc *d, sdr_iq_sums *out)
{
    if (!d || !out)
        return dfail(SDR_ERR_BAD_ARG, "null ddc or output");
    if (!d->sums.on)
        return dfail(SDR_ERR_STATE, "sdr_iq_ddc_read_sums: the sums are off (sdr_iq_ddc_enable_sums)");
    DHIP(hipSetDevice(d->cfg.device_id));
    DHIP(sdr::iq_sums_read(d->sums, out, d->stream));
    return SDR_OK;
}

int sdr_iq_correction_from_sums(const sdr_iq_sums *s, int in_format, sdr_iq_correction *out)
{
    if (!s || !out)
        return dfail(SDR_ERR_BAD_ARG, "null sums or output");
    if (!sdr::iq_correction_from_sums(*s, in_format, out))
        return dfail(SDR_ERR_BAD_ARG, "sdr_iq_correction_from_sums: a format without sums, n < 2, no variance of I, a Q that is a "
                                      "multiple of I, or a value that is not finite");
    return SDR_OK;
}

#pragma GCC visibility pop
}
