// capi_fine.hip — the fine converter behind the C ABI (include/sdrainer_hip.h "fine converter"): an object of its own beside
// the DDC, the channelizer and the bank, with the taps, the NCO table and the carry of n_taps - 1 raw samples of EVERY input
// in device memory.  The kernels are k_fine.hip's; sdr_fine_tune is host/fine_tune.h.
//
// The carry is double-buffered as the DDC's is (capi_ddc.hip): a call's kernel reads carry[cur] and a second small kernel
// behind it forms carry[1 - cur] from carry[cur] and the call's inputs.  The steps and the input map are host state that
// travels with each launch (fine.h FineMap).  Everything is ordered by the object's one stream.  No launcher of another
// object is used or changed here: a process that never creates an sdr_fine launches what it launched.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "fine.h"
#include "host/fine_tune.h"
#include "host/nco_table.h"

namespace sdr {
int set_error(int code, const char *msg);  // capi_bank.hip: feeds sdr_last_error()
}

namespace {

int ffail(int code, const std::string &msg) { return sdr::set_error(code, msg.c_str()); }
#define FHIP(expr)                                                                          \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return ffail(SDR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

bool step_valid(int step) { return step >= -32768 && step <= 32767; }

}  // namespace

struct sdr_fine {
    sdr_fine_config cfg{};
    hipStream_t stream = nullptr;
    sdr::FineMap map{};
    float *d_taps = nullptr;
    float2 *d_nco = nullptr;
    float2 *d_carry[2] = {nullptr, nullptr};  // [n_inputs][n_taps - 1] each
    int cur = 0;            // the carry buffer the next call reads
    int64_t origin = 0;     // index of the first sample
    int64_t total = 0;      // index of the next sample
    bool started = false;   // a process call has been accepted
};

namespace sdr {
const sdr_fine_config &fine_config(const sdr_fine *f) { return f->cfg; }  // chain.h
hipStream_t fine_stream(const sdr_fine *f) { return f->stream; }
}

extern "C" {
#pragma GCC visibility push(default)

int sdr_fine_destroy(sdr_fine *f)
{
    if (!f)
        return SDR_OK;
    (void)hipSetDevice(f->cfg.device_id);
    (void)hipStreamSynchronize(f->stream);
    (void)hipFree(f->d_taps);
    (void)hipFree(f->d_nco);
    (void)hipFree(f->d_carry[0]);
    (void)hipFree(f->d_carry[1]);
    delete f;
    return SDR_OK;
}

int sdr_fine_create(const sdr_fine_config *cfg, const float *taps, const int32_t *nco_steps, const int32_t *inputs, sdr_fine **out)
{
    if (!cfg || !taps || !nco_steps || !out)
        return ffail(SDR_ERR_BAD_ARG, "null config, taps, steps or output");
    if (cfg->struct_size != (int32_t)sizeof(sdr_fine_config))
        return ffail(SDR_ERR_BAD_ARG, "sdr_fine_config.struct_size mismatch");
    if (cfg->n_bands < 1 || cfg->n_bands > sdr::kFineMaxBands)
        return ffail(SDR_ERR_BAD_ARG, "n_bands must be 1 .. 64");
    if (cfg->n_inputs < 1 || cfg->n_inputs > sdr::kFineMaxInputs)
        return ffail(SDR_ERR_BAD_ARG, "n_inputs must be 1 .. 256");
    if (cfg->decimation < 1 || cfg->decimation > sdr::kDdcMaxDecimation)
        return ffail(SDR_ERR_BAD_ARG, "decimation must be 1 .. 256");
    if (cfg->n_taps < 1 || cfg->n_taps > sdr::kDdcMaxTaps)
        return ffail(SDR_ERR_BAD_ARG, "n_taps must be 1 .. 4096");
    if (cfg->max_in_samples < cfg->decimation || cfg->max_in_samples % cfg->decimation != 0)
        return ffail(SDR_ERR_BAD_ARG, "max_in_samples must be a positive multiple of the decimation");
    if (cfg->reserved != 0)
        return ffail(SDR_ERR_BAD_ARG, "sdr_fine_config.reserved must be 0");
    if (!inputs && cfg->n_bands > cfg->n_inputs)
        return ffail(SDR_ERR_BAD_ARG, "without an input map band b reads input b: n_bands must not exceed n_inputs");
    for (int b = 0; b < cfg->n_bands; b++) {
        if (!step_valid(nco_steps[b]))
            return ffail(SDR_ERR_BAD_ARG, "an NCO step must lie in [-32768, 32767]");
        if (inputs && (inputs[b] < 0 || inputs[b] >= cfg->n_inputs))
            return ffail(SDR_ERR_BAD_ARG, "an input index must lie in 0 .. n_inputs - 1");
    }
    FHIP(hipSetDevice(cfg->device_id));
    sdr_fine *f = new sdr_fine();
    f->cfg = *cfg;
    for (int b = 0; b < cfg->n_bands; b++) {
        f->map.step[b] = (int16_t)nco_steps[b];
        f->map.input[b] = (uint8_t)(inputs ? inputs[b] : b);
    }
    // (a failure half way frees what was allocated so far: sdr_fine_destroy tolerates null members)
#define FCREATE(expr)                                                                       \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess) {                                                             \
            const std::string _msg = std::string(#expr) + ": " + hipGetErrorString(_e);     \
            sdr_fine_destroy(f);                                                            \
            return ffail(SDR_ERR_HIP, _msg);                                                \
        }                                                                                   \
    } while (0)
    const size_t T = (size_t)cfg->n_taps, keep = T > 1 ? T - 1 : 1;
    const size_t carry_bytes = sizeof(float2) * keep * (size_t)cfg->n_inputs;
    FCREATE(hipMalloc((void **)&f->d_taps, sizeof(float) * T));
    FCREATE(hipMalloc((void **)&f->d_nco, sizeof(float2) * (size_t)sdr::kDdcNco));
    for (int i = 0; i < 2; i++) {
        FCREATE(hipMalloc((void **)&f->d_carry[i], carry_bytes));
        FCREATE(hipMemset(f->d_carry[i], 0, carry_bytes));
    }
    std::vector<float> co((size_t)sdr::kDdcNco), si((size_t)sdr::kDdcNco);
    sdr::build_nco(co.data(), si.data());
    std::vector<float2> tab((size_t)sdr::kDdcNco);
    for (size_t i = 0; i < tab.size(); i++)
        tab[i] = make_float2(co[i], si[i]);
    FCREATE(hipMemcpy(f->d_nco, tab.data(), sizeof(float2) * tab.size(), hipMemcpyHostToDevice));
    FCREATE(hipMemcpy(f->d_taps, taps, sizeof(float) * T, hipMemcpyHostToDevice));
#undef FCREATE
    *out = f;
    return SDR_OK;
}

int sdr_fine_sync(sdr_fine *f)
{
    if (!f)
        return ffail(SDR_ERR_BAD_ARG, "null fine converter");
    FHIP(hipSetDevice(f->cfg.device_id));
    FHIP(hipStreamSynchronize(f->stream));
    return SDR_OK;
}

int sdr_fine_set_stream(sdr_fine *f, void *hip_stream)
{
    if (!f)
        return ffail(SDR_ERR_BAD_ARG, "null fine converter");
    FHIP(hipSetDevice(f->cfg.device_id));
    FHIP(hipStreamSynchronize(f->stream));  // (the carry of the calls so far is ordered by the old stream)
    f->stream = (hipStream_t)hip_stream;
    return SDR_OK;
}

int sdr_fine_set_first_sample(sdr_fine *f, int64_t k0)
{
    if (!f)
        return ffail(SDR_ERR_BAD_ARG, "null fine converter");
    if (f->started)
        return ffail(SDR_ERR_STATE, "sdr_fine_set_first_sample: samples have been processed (call it right after sdr_fine_create)");
    if (k0 < 0 || k0 % f->cfg.decimation != 0)
        return ffail(SDR_ERR_BAD_ARG, "the first sample must be >= 0 and a multiple of the decimation");
    f->origin = f->total = k0;
    return SDR_OK;
}

int64_t sdr_fine_total_samples(sdr_fine *f) { return f ? f->total : 0; }

int sdr_fine_set_nco_step(sdr_fine *f, int band, int step)
{
    if (!f)
        return ffail(SDR_ERR_BAD_ARG, "null fine converter");
    if (band < 0 || band >= f->cfg.n_bands)
        return ffail(SDR_ERR_BAD_ARG, "band out of range");
    if (!step_valid(step))
        return ffail(SDR_ERR_BAD_ARG, "an NCO step must lie in [-32768, 32767]");
    f->map.step[band] = (int16_t)step;
    return SDR_OK;
}

int sdr_fine_set_input(sdr_fine *f, int band, int input)
{
    if (!f)
        return ffail(SDR_ERR_BAD_ARG, "null fine converter");
    if (band < 0 || band >= f->cfg.n_bands)
        return ffail(SDR_ERR_BAD_ARG, "band out of range");
    if (input < 0 || input >= f->cfg.n_inputs)
        return ffail(SDR_ERR_BAD_ARG, "an input index must lie in 0 .. n_inputs - 1");
    f->map.input[band] = (uint8_t)input;
    return SDR_OK;
}

int sdr_fine_process_device(sdr_fine *f, const float *in_dev, size_t in_stride_samples, size_t n_in_samples, float *out_dev,
                            size_t band_stride_samples)
{
    if (!f || !in_dev || !out_dev)
        return ffail(SDR_ERR_BAD_ARG, "null fine converter, input or output");
    const sdr_fine_config &c = f->cfg;
    const size_t D = (size_t)c.decimation;
    if (n_in_samples == 0 || n_in_samples % D != 0 || n_in_samples > (size_t)c.max_in_samples)
        return ffail(SDR_ERR_BAD_SIZE, "n_in_samples must be a positive multiple of the decimation, at most max_in_samples");
    if (((uintptr_t)in_dev & 15u) || ((uintptr_t)out_dev & 15u))
        return ffail(SDR_ERR_BAD_ARG, "in_dev and out_dev must be 16-byte aligned");
    if (in_stride_samples % 4 != 0 || in_stride_samples < n_in_samples)
        return ffail(SDR_ERR_BAD_ARG, "in_stride_samples must be a multiple of 4 and at least n_in_samples");
    if (band_stride_samples % 4 != 0 || band_stride_samples < n_in_samples / D)
        return ffail(SDR_ERR_BAD_ARG, "band_stride_samples must be a multiple of 4 and at least the outputs per band");
    FHIP(hipSetDevice(c.device_id));
    sdr::FineLaunch l{};
    l.in = reinterpret_cast<const float2 *>(in_dev);
    l.in_stride = in_stride_samples;
    l.carry = f->d_carry[f->cur];
    l.nco = f->d_nco;
    l.taps = f->d_taps;
    l.out = out_dev;
    l.out_stride = band_stride_samples;
    l.first = f->total;
    l.origin = f->origin;
    l.n_in = (int)n_in_samples;
    l.n_bands = c.n_bands;
    l.n_inputs = c.n_inputs;
    l.decimation = c.decimation;
    l.n_taps = c.n_taps;
    l.map = f->map;
    FHIP(sdr::launch_fine(l, f->stream));
    FHIP(sdr::launch_fine_carry(f->d_carry[f->cur], l.in, in_stride_samples, (int)n_in_samples, c.n_inputs, c.n_taps,
                                f->d_carry[1 - f->cur], f->stream));
    f->cur = 1 - f->cur;
    f->total += (int64_t)n_in_samples;
    f->started = true;
    return SDR_OK;
}

int sdr_fine_tune(int n_channels, int decimation, int64_t target, int32_t *channel, int32_t *step)
{
    if (!channel || !step)
        return ffail(SDR_ERR_BAD_ARG, "null channel or step output");
    if (!sdr::fine_tune(n_channels, decimation, target, channel, step))
        return ffail(SDR_ERR_BAD_ARG, "sdr_fine_tune: n_channels must be a power of two in 2 .. 256, decimation one of M, M/2, M/4 "
                                      "and at least 1, and |target| at most 32768 * decimation");
    return SDR_OK;
}

#pragma GCC visibility pop
}
