// host/iq_sums.h — the host side of the raw-stream sums (include/sdrainer_hip.h "IQ correction") as plain arithmetic: which
// formats are summed, the integer unit u = a * b + c of a raw byte or word, the scale S of that unit, the bookkeeping of n
// and skipped around 2^32, and sdr_iq_correction_from_sums' float64 sequence.  No HIP include: capi_ddc.hip, capi_chan.hip
// and k_iq_sums.hip use it, tests/host/test_iq_sums_host.cpp walks it on the host.
#pragma once
#include <cmath>
#include <cstdint>

#include "ddc_format.h"

namespace sdr {

// sums are offered for the three complex integer formats
constexpr bool iq_sums_format(int fmt) { return fmt == SDR_DDC_CS8 || fmt == SDR_DDC_CU8 || fmt == SDR_DDC_SC16; }

// value = u / S: cs8 x / 128, cu8 (2 x - 255) / 256, sc16 x / 32767
constexpr double iq_unit_scale(int fmt) { return fmt == SDR_DDC_CS8 ? 128.0 : fmt == SDR_DDC_CU8 ? 256.0 : 32767.0; }

// The kernel sums b = byte ^ flip as an unsigned value 0 .. 255 for both 8-bit formats (iq8.h: cs8's x ^ 0x80 is x + 128) and
// the int16 itself for sc16; the unit is u = a * b + c.
struct IqUnit {
    int a, c;
};
constexpr IqUnit iq_unit(int fmt) { return fmt == SDR_DDC_CS8 ? IqUnit{1, -128} : fmt == SDR_DDC_CU8 ? IqUnit{2, -255} : IqUnit{1, 0}; }

// the sums of n values of u from the sums of b: exact in int64 (n <= 2^31 per call, b^2 < 2^30)
struct IqRawSums {
    int64_t i, q, ii, qq, iq;
};
constexpr IqRawSums iq_unit_sums(IqRawSums s, IqUnit u, int64_t n)
{
    const int64_t a = u.a, c = u.c;
    return IqRawSums{a * s.i + c * n, a * s.q + c * n, a * a * s.ii + 2 * a * c * s.i + c * c * n, a * a * s.qq + 2 * a * c * s.q + c * c * n,
                     a * a * s.iq + a * c * (s.i + s.q) + c * c * n};
}

// n and skipped since the last read: a call that would take n past 2^32 is not summed, so that sum_ii <= 2^32 * 2^30
constexpr int64_t kIqSumsMaxN = (int64_t)1 << 32;
struct IqSumsCount {
    int64_t n = 0, skipped = 0;
    // true: the call's samples are summed
    bool accept(int64_t n_call)
    {
        if (n_call > kIqSumsMaxN - n) {
            skipped += n_call;
            return false;
        }
        n += n_call;
        return true;
    }
    void clear() { n = skipped = 0; }
};

// sdr_iq_correction_from_sums: every line one float64 operation, rounded once (no contraction: -ffp-contract=off).  false:
// refused, *out untouched.
inline bool iq_correction_from_sums(const sdr_iq_sums &s, int fmt, sdr_iq_correction *out)
{
    if (!iq_sums_format(fmt) || s.n < 2)
        return false;
    const double N = (double)s.n;
    const double mi = (double)s.sum_i / N, mq = (double)s.sum_q / N;
    const double mimi = mi * mi, mqmq = mq * mq, mimq = mi * mq;
    const double vi = (double)s.sum_ii / N - mimi;
    const double vq = (double)s.sum_qq / N - mqmq;
    const double c = (double)s.sum_iq / N - mimq;
    if (!(vi > 0.0))
        return false;
    const double cc = c * c;
    const double r = vq - cc / vi;
    if (!(r > 0.0))
        return false;
    const double g = std::sqrt(vi / r);
    const double x = -(g * (c / vi));
    const double S = iq_unit_scale(fmt);
    const double dre = mi / S, dim = mq / S;
    if (!std::isfinite(g) || !std::isfinite(x) || !std::isfinite(dre) || !std::isfinite(dim) || !std::isfinite(vq))
        return false;
    out->dc_re = (float)dre;
    out->dc_im = (float)dim;
    out->gain_im = (float)g;
    out->cross = (float)x;
    return true;
}

}  // namespace sdr
