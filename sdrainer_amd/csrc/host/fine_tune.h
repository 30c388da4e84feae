// host/fine_tune.h — where to point a fine converter's band behind a channelizer (include/sdrainer_hip.h "fine converter",
// sdr_fine_tune), as plain integer arithmetic.  No HIP include: capi_fine.hip uses it, tests/host/fine_tune_main.cpp walks it
// on the host.
//
// Behind a channelizer of M channels with decimation D a fine step tunes by step * (wide_rate / D) / 65536, so the unit of
// `target` is wide_rate / (65536 * D) and channel c's centre c * wide_rate / M is c * q units, q = 65536 * D / M.  M divides
// 65536, so q is an integer: 65536, 32768 or 16384 for D = M, M/2, M/4.
#pragma once
#include <cstdint>

namespace sdr {

constexpr int kFineTuneMaxChannels = 256;
constexpr int64_t kFineTuneNco = 65536;

// the channelizer's rule for (M, D) (chan.h chan_log_m, without the taps): M a power of two in 2 .. 256, D one of M, M/2,
// M/4 and at least 1
constexpr bool fine_tune_geometry(int m, int d)
{
    return m >= 2 && m <= kFineTuneMaxChannels && (m & (m - 1)) == 0 && d >= 1 && (d == m || d * 2 == m || d * 4 == m);
}

// the floor of a / b for b > 0
constexpr int64_t fine_floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0 && a < 0) ? 1 : 0); }

// false, with the outputs untouched, for an illegal geometry or a target outside the wide stream (|target| > 32768 * D)
inline bool fine_tune(int m, int d, int64_t target, int32_t *channel, int32_t *step)
{
    if (!fine_tune_geometry(m, d))
        return false;
    const int64_t half = (kFineTuneNco / 2) * d;  // the wide stream's edge in target units
    if (target < -half || target > half)
        return false;
    const int64_t q = kFineTuneNco * d / m;
    // nearest channel: floor((2 target + q) / (2 q)) rounds a tie up; a tie goes to the even channel
    int64_t c = fine_floor_div(2 * target + q, 2 * q);
    if ((2 * target + q) % (2 * q) == 0 && (c & 1) != 0)
        c--;
    int64_t s = target - c * q;  // in [-q/2, q/2]
    if (s == kFineTuneNco / 2) {  // q = 65536 only: the step's range ends at 32767
        c++;
        s = -kFineTuneNco / 2;
    }
    *channel = (int32_t)(((c % m) + m) % m);
    *step = (int32_t)s;
    return true;
}

}  // namespace sdr
