// capi_fine.hip — the fine converter behind the C ABI (include/sdrainer_hip.h "fine converter"): an object of its own beside
// the DDC, the channelizer and the bank, with the taps, the NCO table and the carry of n_taps - 1 raw samples of EVERY input
// in device memory.  The kernels are k_fine.hip's; sdr_fine_tune is host/fine_tune.h.
//
// The stream and the sample clock, the double-buffered carry (a call's kernel reads its current half and a second small
// kernel behind it forms the other from that and the call's inputs) and the first checks of a call are front.h's.  The steps
// and the input map are host state that travels with each launch (fine.h FineMap).  Everything is ordered by the object's
// one stream.  No launcher of another object is used or changed here: a process that never creates an sdr_fine launches
// what it launched.
#include "fine.h"
#include "front.h"
#include "host/fine_tune.h"

using sdr::fail;

struct sdr_fine : sdr::FrontObject {
    sdr_fine_config cfg{};
    sdr::FineMap map{};
    float *d_taps = nullptr;
    float2 *d_nco = nullptr;
    sdr::RawCarry carry;  // float2 [n_inputs][n_taps - 1] each
};

namespace sdr {
const sdr_fine_config &fine_config(const sdr_fine *f) { return f->cfg; }  // chain.h
hipStream_t fine_stream(const sdr_fine *f) { return f->stream; }
}

namespace {

const sdr::CallTexts kCall = {"null fine converter, input or output",
                              "n_in_samples must be a positive multiple of the decimation, at most max_in_samples",
                              "in_dev and out_dev must be 16-byte aligned"};

}  // namespace

extern "C" {
#pragma GCC visibility push(default)

int sdr_fine_destroy(sdr_fine *f)
{
    if (!f)
        return SDR_OK;
    f->quiesce();
    (void)hipFree(f->d_taps);
    (void)hipFree(f->d_nco);
    f->carry.release();
    delete f;
    return SDR_OK;
}

int sdr_fine_create(const sdr_fine_config *cfg, const float *taps, const int32_t *nco_steps, const int32_t *inputs, sdr_fine **out)
{
    if (!cfg || !taps || !nco_steps || !out)
        return fail(SDR_ERR_BAD_ARG, "null config, taps, steps or output");
    if (cfg->struct_size != (int32_t)sizeof(sdr_fine_config))
        return fail(SDR_ERR_BAD_ARG, "sdr_fine_config.struct_size mismatch");
    if (cfg->n_bands < 1 || cfg->n_bands > sdr::kFineMaxBands)
        return fail(SDR_ERR_BAD_ARG, "n_bands must be 1 .. 64");
    if (cfg->n_inputs < 1 || cfg->n_inputs > sdr::kFineMaxInputs)
        return fail(SDR_ERR_BAD_ARG, "n_inputs must be 1 .. 256");
    if (cfg->decimation < 1 || cfg->decimation > sdr::kDdcMaxDecimation)
        return fail(SDR_ERR_BAD_ARG, "decimation must be 1 .. 256");
    if (cfg->n_taps < 1 || cfg->n_taps > sdr::kDdcMaxTaps)
        return fail(SDR_ERR_BAD_ARG, "n_taps must be 1 .. 4096");
    if (cfg->max_in_samples < cfg->decimation || cfg->max_in_samples % cfg->decimation != 0)
        return fail(SDR_ERR_BAD_ARG, "max_in_samples must be a positive multiple of the decimation");
    if (cfg->reserved != 0)
        return fail(SDR_ERR_BAD_ARG, "sdr_fine_config.reserved must be 0");
    if (!inputs && cfg->n_bands > cfg->n_inputs)
        return fail(SDR_ERR_BAD_ARG, "without an input map band b reads input b: n_bands must not exceed n_inputs");
    for (int b = 0; b < cfg->n_bands; b++) {
        if (!sdr::step_valid(nco_steps[b]))
            return fail(SDR_ERR_BAD_ARG, "an NCO step must lie in [-32768, 32767]");
        if (inputs && (inputs[b] < 0 || inputs[b] >= cfg->n_inputs))
            return fail(SDR_ERR_BAD_ARG, "an input index must lie in 0 .. n_inputs - 1");
    }
    HIP_TRY(hipSetDevice(cfg->device_id));
    sdr::Building<sdr_fine, sdr_fine_destroy> f(new sdr_fine());
    f->cfg = *cfg;
    f->place(cfg->device_id, cfg->decimation, cfg->max_in_samples);
    for (int b = 0; b < cfg->n_bands; b++) {
        f->map.step[b] = (int16_t)nco_steps[b];
        f->map.input[b] = (uint8_t)(inputs ? inputs[b] : b);
    }
    HIP_TRY(hipMalloc((void **)&f->d_taps, sizeof(float) * (size_t)cfg->n_taps));
    HIP_TRY(hipMalloc((void **)&f->d_nco, sizeof(float2) * (size_t)sdr::kDdcNco));
    int rc = f->carry.alloc(sizeof(float2) * sdr::carry_samples(cfg->n_taps) * (size_t)cfg->n_inputs);
    if (rc || (rc = sdr::upload_coefficients(f->d_taps, f->d_nco, taps, cfg->n_taps)))
        return rc;
    *out = f.release();
    return SDR_OK;
}

int sdr_fine_sync(sdr_fine *f) { return sdr::front_sync(f, "null fine converter"); }

int sdr_fine_set_stream(sdr_fine *f, void *hip_stream) { return sdr::front_set_stream(f, hip_stream, "null fine converter"); }

int sdr_fine_set_first_sample(sdr_fine *f, int64_t k0)
{
    return sdr::front_set_first_sample(f, k0, "null fine converter",
                                       "sdr_fine_set_first_sample: samples have been processed (call it right after sdr_fine_create)",
                                       "the first sample must be >= 0 and a multiple of the decimation");
}

int64_t sdr_fine_total_samples(sdr_fine *f) { return sdr::front_total_samples(f); }

int sdr_fine_set_nco_step(sdr_fine *f, int band, int step)
{
    if (!f)
        return fail(SDR_ERR_BAD_ARG, "null fine converter");
    if (band < 0 || band >= f->cfg.n_bands)
        return fail(SDR_ERR_BAD_ARG, "band out of range");
    if (!sdr::step_valid(step))
        return fail(SDR_ERR_BAD_ARG, "an NCO step must lie in [-32768, 32767]");
    f->map.step[band] = (int16_t)step;
    return SDR_OK;
}

int sdr_fine_set_input(sdr_fine *f, int band, int input)
{
    if (!f)
        return fail(SDR_ERR_BAD_ARG, "null fine converter");
    if (band < 0 || band >= f->cfg.n_bands)
        return fail(SDR_ERR_BAD_ARG, "band out of range");
    if (input < 0 || input >= f->cfg.n_inputs)
        return fail(SDR_ERR_BAD_ARG, "an input index must lie in 0 .. n_inputs - 1");
    f->map.input[band] = (uint8_t)input;
    return SDR_OK;
}

int sdr_fine_process_device(sdr_fine *f, const float *in_dev, size_t in_stride_samples, size_t n_in_samples, float *out_dev,
                            size_t band_stride_samples)
{
    const int rc = sdr::check_call(f, in_dev, n_in_samples, out_dev, true, kCall);
    if (rc)
        return rc;
    const sdr_fine_config &c = f->cfg;
    if (!sdr::stride_ok(in_stride_samples, n_in_samples))
        return fail(SDR_ERR_BAD_ARG, "in_stride_samples must be a multiple of 4 and at least n_in_samples");
    if (!sdr::stride_ok(band_stride_samples, n_in_samples / (size_t)c.decimation))
        return fail(SDR_ERR_BAD_ARG, "band_stride_samples must be a multiple of 4 and at least the outputs per band");
    HIP_TRY(hipSetDevice(f->device_id));
    sdr::FineLaunch l{};
    l.in = reinterpret_cast<const float2 *>(in_dev);
    l.in_stride = in_stride_samples;
    l.carry = static_cast<const float2 *>(f->carry.cur());
    l.nco = f->d_nco;
    l.taps = f->d_taps;
    l.out = out_dev;
    l.out_stride = band_stride_samples;
    l.first = f->clock.total;
    l.origin = f->clock.origin;
    l.n_in = (int)n_in_samples;
    l.n_bands = c.n_bands;
    l.n_inputs = c.n_inputs;
    l.decimation = c.decimation;
    l.n_taps = c.n_taps;
    l.map = f->map;
    HIP_TRY(sdr::launch_fine(l, f->stream));
    HIP_TRY(sdr::launch_fine_carry(l.carry, l.in, in_stride_samples, (int)n_in_samples, c.n_inputs, c.n_taps,
                                   static_cast<float2 *>(f->carry.next()), f->stream));
    f->carry.flip();
    f->clock.advance(n_in_samples);
    return SDR_OK;
}

int sdr_fine_tune(int n_channels, int decimation, int64_t target, int32_t *channel, int32_t *step)
{
    if (!channel || !step)
        return fail(SDR_ERR_BAD_ARG, "null channel or step output");
    if (!sdr::fine_tune(n_channels, decimation, target, channel, step))
        return fail(SDR_ERR_BAD_ARG, "sdr_fine_tune: n_channels must be a power of two in 2 .. 256, decimation one of M, M/2, M/4 "
                                     "and at least 1, and |target| at most 32768 * decimation");
    return SDR_OK;
}

#pragma GCC visibility pop
}
