// front.h — the host core of the front-end objects behind the C ABI: what capi_ddc.hip, capi_chan.hip, capi_fine.hip,
// capi_nb.hip and capi_chain.hip share.  "An object on a stream with a sample clock" is defined here once: the failure
// function and the HIP-error macro (bank.h uses the same two), the guard that destroys a half-built object, FrontObject
// (device, stream, SampleClock), HostUpload (process_host's way through pinned memory), RawCarry (the double-buffered
// history of n_taps - 1 samples), the coefficient upload, the IQ state of the two stage-one objects and the checks of a
// process call.  The integer rules are host/front_rules.h's; every message text stays in the capi file that reports it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/sdrainer_hip.h"
#include "ddc.h"
#include "host/ddc_format.h"
#include "host/front_rules.h"
#include "host/nco_table.h"
#include "iq_sums_dev.h"

namespace sdr {

int set_error(int code, const char *msg);  // capi_bank.hip: the single feed of sdr_last_error()

inline int fail(int code, const std::string &msg) { return set_error(code, msg.c_str()); }

}  // namespace sdr

// in a function that returns a status: a HIP call that fails ends it with SDR_ERR_HIP and the call's text
#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return ::sdr::fail(SDR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));        \
    } while (0)

namespace sdr {

// What *_create holds the new object in until it succeeds: leaving early destroys it with the object's own sdr_*_destroy,
// which tolerates null members.  (HIP_TRY has set the error text by then: a return's value is formed before locals go.)
template <class T, int (*Destroy)(T *)>
struct DestroyWith {
    void operator()(T *p) const { (void)Destroy(p); }
};
template <class T, int (*Destroy)(T *)>
using Building = std::unique_ptr<T, DestroyWith<T, Destroy>>;

struct FrontObject {
    int device_id = 0;
    hipStream_t stream = nullptr;
    SampleClock clock;

    void place(int device, int64_t unit, int64_t max_in)
    {
        device_id = device;
        clock.unit = unit;
        clock.max_in = max_in;
    }
    int sync() const
    {
        HIP_TRY(hipSetDevice(device_id));
        HIP_TRY(hipStreamSynchronize(stream));
        return SDR_OK;
    }
    int set_stream(void *hip_stream)
    {
        const int rc = sync();  // (the state the calls so far left is ordered by the old stream)
        if (rc == SDR_OK)
            stream = (hipStream_t)hip_stream;
        return rc;
    }
    // destroy's first step: whatever is in flight finishes before its memory goes
    void quiesce() const
    {
        (void)hipSetDevice(device_id);
        (void)hipStreamSynchronize(stream);
    }
};

// the four entry points every object has, given its texts
inline int front_sync(const FrontObject *o, const char *null_text) { return o ? o->sync() : fail(SDR_ERR_BAD_ARG, null_text); }
inline int front_set_stream(FrontObject *o, void *hip_stream, const char *null_text)
{
    return o ? o->set_stream(hip_stream) : fail(SDR_ERR_BAD_ARG, null_text);
}
inline int front_set_first_sample(FrontObject *o, int64_t k0, const char *null_text, const char *state_text, const char *arg_text)
{
    if (!o)
        return fail(SDR_ERR_BAD_ARG, null_text);
    switch (o->clock.set_first(k0)) {
    case SampleClock::State:
        return fail(SDR_ERR_STATE, state_text);
    case SampleClock::BadArg:
        return fail(SDR_ERR_BAD_ARG, arg_text);
    default:
        return SDR_OK;
    }
}
inline int64_t front_total_samples(const FrontObject *o) { return o ? o->clock.total : 0; }

// The first three checks of every process call, in this order: null, length, alignment.  (A host pointer needs no
// alignment.)  What follows - strides, overlap - is the caller's.
struct CallTexts {
    const char *null_args, *length, *alignment;
};
inline int check_call(const FrontObject *o, const void *in, size_t n_in, const void *out, bool in_on_device, const CallTexts &t)
{
    if (!o || !in || !out)
        return fail(SDR_ERR_BAD_ARG, t.null_args);
    if (o->clock.check_len(n_in) != SampleClock::Ok)
        return fail(SDR_ERR_BAD_SIZE, t.length);
    if ((in_on_device && !aligned16(in)) || !aligned16(out))
        return fail(SDR_ERR_BAD_ARG, t.alignment);
    return SDR_OK;
}

// A process_host call's upload through pinned memory.  Nothing is allocated before the first such call; a failed
// allocation leaves the object usable (what was allocated stays and is reused).
struct HostUpload {
    void *h_pin = nullptr;
    void *d_in = nullptr;  // the device buffer of an object that uploads into one of its own
    hipEvent_t uploaded = nullptr;

    // allocates what is missing, then waits until the last upload has left the pinned buffer
    int ready(size_t capacity, bool own_device_buffer)
    {
        if (own_device_buffer && !d_in)
            HIP_TRY(hipMalloc(&d_in, capacity));
        if (!h_pin)
            HIP_TRY(hipHostMalloc(&h_pin, capacity, hipHostMallocDefault));
        if (!uploaded)
            HIP_TRY(hipEventCreateWithFlags(&uploaded, hipEventDisableTiming));
        else
            HIP_TRY(hipEventSynchronize(uploaded));
        return SDR_OK;
    }
    int send(const void *src, size_t bytes, void *dst_dev, hipStream_t stream)
    {
        memcpy(h_pin, src, bytes);
        HIP_TRY(hipMemcpyAsync(dst_dev, h_pin, bytes, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipEventRecord(uploaded, stream));
        return SDR_OK;
    }
    // both; dst_dev == nullptr: into d_in
    int stage(const void *src, size_t bytes, size_t capacity, void *dst_dev, hipStream_t stream)
    {
        const int rc = ready(capacity, dst_dev == nullptr);
        return rc ? rc : send(src, bytes, dst_dev ? dst_dev : d_in, stream);
    }
    void release()
    {
        (void)hipFree(d_in);
        if (h_pin)
            (void)hipHostFree(h_pin);
        if (uploaded)
            (void)hipEventDestroy(uploaded);
    }
};

// The raw history between calls, double-buffered: a call's kernel reads cur() and a small kernel behind it forms next()
// from cur() and the call's input - also where the call is shorter than the history and part of it survives.
struct RawCarry {
    void *buf[2] = {nullptr, nullptr};
    int at = 0;

    int alloc(size_t bytes)
    {
        for (int i = 0; i < 2; i++) {
            HIP_TRY(hipMalloc(&buf[i], bytes));
            HIP_TRY(hipMemset(buf[i], 0, bytes));
        }
        return SDR_OK;
    }
    void *cur() const { return buf[at]; }
    void *next() const { return buf[1 - at]; }
    void flip() { at = 1 - at; }
    void release()
    {
        (void)hipFree(buf[0]);
        (void)hipFree(buf[1]);
    }
};

inline size_t carry_samples(int n_taps) { return n_taps > 1 ? (size_t)n_taps - 1 : 1; }

// the NCO table (host/nco_table.h) as (cos, sin) pairs and the taps, into buffers the caller allocated
inline int upload_coefficients(float *d_taps, float2 *d_nco, const float *taps, int n_taps)
{
    std::vector<float> co((size_t)kDdcNco), si((size_t)kDdcNco);
    build_nco(co.data(), si.data());
    std::vector<float2> tab((size_t)kDdcNco);
    for (size_t i = 0; i < tab.size(); i++)
        tab[i] = make_float2(co[i], si[i]);
    HIP_TRY(hipMemcpy(d_nco, tab.data(), sizeof(float2) * tab.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_taps, taps, sizeof(float) * (size_t)n_taps, hipMemcpyHostToDevice));
    return SDR_OK;
}

// The IQ state of a stage-one object: the correction its kernel applies while one is set, and the raw stream's sums.
struct IqFront {
    bool corrected = false;
    sdr_iq_correction corr{};
    IqSums sums;

    // behind the object's own kernel, in this order: the carry's kernel, the sums of the call's input where they are on,
    // and only then the flip
    int after_launch(int fmt, RawCarry &carry, const void *in, int n_in, int n_taps, hipStream_t stream)
    {
        HIP_TRY(launch_ddc_carry(fmt, carry.cur(), in, n_in, n_taps, carry.next(), stream));
        if (sums.on)
            HIP_TRY(iq_sums_add(sums, fmt, in, n_in, stream));
        carry.flip();
        return SDR_OK;
    }
};

// sdr_iq_{ddc,chan}_*: T is a FrontObject with an IqFront `iq` and a config with in_format and max_in_samples
struct IqTexts {
    const char *null_object, *null_output, *real_format, *not_finite, *no_sums_format, *sums_off;
};
template <class T>
int iq_set_correction(T *o, const sdr_iq_correction *c, const IqTexts &t)
{
    if (!o)
        return fail(SDR_ERR_BAD_ARG, t.null_object);
    if (ddc_is_real(o->cfg.in_format))
        return fail(SDR_ERR_BAD_ARG, t.real_format);
    if (c && !(std::isfinite(c->dc_re) && std::isfinite(c->dc_im) && std::isfinite(c->gain_im) && std::isfinite(c->cross)))
        return fail(SDR_ERR_BAD_ARG, t.not_finite);
    o->iq.corrected = c != nullptr;
    o->iq.corr = c ? *c : sdr_iq_correction{};
    return SDR_OK;
}
template <class T>
int iq_enable_sums(T *o, int on, const IqTexts &t)
{
    if (!o)
        return fail(SDR_ERR_BAD_ARG, t.null_object);
    if (!iq_sums_format(o->cfg.in_format))
        return fail(SDR_ERR_BAD_ARG, t.no_sums_format);
    HIP_TRY(hipSetDevice(o->device_id));
    HIP_TRY(iq_sums_enable(o->iq.sums, o->cfg.in_format, o->cfg.max_in_samples, on != 0, o->stream));
    return SDR_OK;
}
template <class T>
int iq_read_sums(T *o, sdr_iq_sums *out, const IqTexts &t)
{
    if (!o || !out)
        return fail(SDR_ERR_BAD_ARG, t.null_output);
    if (!o->iq.sums.on)
        return fail(SDR_ERR_STATE, t.sums_off);
    HIP_TRY(hipSetDevice(o->device_id));
    HIP_TRY(iq_sums_read(o->iq.sums, out, o->stream));
    return SDR_OK;
}

}  // namespace sdr
