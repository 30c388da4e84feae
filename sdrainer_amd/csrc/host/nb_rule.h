// host/nb_rule.h — the impulse noise blanker's integer rule (include/sdrainer_hip.h "impulse noise blanker") as plain
// arithmetic: which formats are blanked, the unit u of a raw value, a sample's squared magnitude m, the inequality that
// makes a sample an impulse, the per-block threshold the kernels compare m with, the blank word, the limits of a
// configuration, and the whole definition over one stream (sdr_nb_blank_host).  No HIP include: capi_nb.hip and k_nb.hip
// use it, tests/host/nb_rule_main.cpp walks it on the host.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ddc_format.h"

#if defined(__HIPCC__)
#define SDR_NB_HD __host__ __device__
#else
#define SDR_NB_HD
#endif

namespace sdr {

constexpr int kNbMinBlock = 64, kNbMaxBlock = 4096, kNbMaxWindow = 64, kNbMaxSpan = 65536;  // B, W, B * W
constexpr int kNbMinRatio = 16, kNbMaxRatio = 16384;                                          // ratio_q4 (0: off)

// the six integer formats; float32 streams are out of scope
constexpr bool nb_format(int fmt) { return ddc_format_valid(fmt) && ddc_complex_base(fmt) != SDR_DDC_F32; }
constexpr bool nb_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }
constexpr bool nb_geometry(int block, int window)
{
    return nb_pow2(block) && nb_pow2(window) && block >= kNbMinBlock && block <= kNbMaxBlock && window <= kNbMaxWindow &&
           (long long)block * window <= kNbMaxSpan;
}
constexpr bool nb_threshold_valid(int block, int ratio_q4, int hold)
{
    return (ratio_q4 == 0 || (ratio_q4 >= kNbMinRatio && ratio_q4 <= kNbMaxRatio)) && hold >= 0 && hold <= block;
}
constexpr int nb_log2(int v) { return v <= 1 ? 0 : 1 + nb_log2(v >> 1); }

// The inequality's two sides in unsigned 64 bits.  The largest sample is sc16 (-32768, -32768): m = 2^31, so the left side
// is at most 2^31 * 2^16 * 2^4 = 2^51; a block's power is at most B * 2^31, R at most B * W * 2^31 = 2^47, and the right
// side at most 2^14 * 2^47 = 2^61.
constexpr uint64_t kNbMaxM = 2ull * 32768 * 32768;
static_assert(kNbMaxM * kNbMaxSpan * 16 < (1ull << 52), "the left side stays below 2^52");
static_assert((uint64_t)kNbMaxRatio * (kNbMaxM * kNbMaxSpan) < (1ull << 62), "the right side stays below 2^62");
static_assert(kNbMaxM * kNbMaxBlock <= (1ull << 43), "a block's power is at most 2^43");

// sample k of a judged block with reference level R is an impulse iff this holds (ratio_q4 == 0: never)
SDR_NB_HD constexpr bool nb_is_impulse(uint64_t m, int span, int ratio_q4, uint64_t R)
{
    return ratio_q4 != 0 && m * (uint64_t)span * 16u > (uint64_t)ratio_q4 * R;
}

// The same decision with one shift per block: m * C > X  <=>  m > floor(X / C) for integers and C > 0, and C = span * 16 is
// a power of two.  m <= 2^31, so a quotient of 2^32 - 1 or more means "never", which is also what an unjudged block and
// ratio_q4 == 0 get.
constexpr uint32_t kNbNever = 0xffffffffu;
SDR_NB_HD constexpr uint32_t nb_threshold(uint64_t R, int ratio_q4, int span_log2, bool judged)
{
    if (!judged || ratio_q4 == 0)
        return kNbNever;
    const uint64_t q = ((uint64_t)ratio_q4 * R) >> (span_log2 + 4);
    return q >= kNbNever ? kNbNever : (uint32_t)q;
}
SDR_NB_HD constexpr bool nb_over(uint32_t m, uint32_t threshold) { return m > threshold; }

// the unit of one raw value of a format's sample type: x for int8 and int16, 2 x - 255 for uint8
SDR_NB_HD constexpr int nb_unit_u8(uint32_t byte) { return 2 * (int)byte - 255; }

// m of sample k of a raw stream, from host memory
inline uint64_t nb_mag_host(const void *raw, int fmt, size_t k)
{
    const int base = ddc_complex_base(fmt), parts = ddc_is_real(fmt) ? 1 : 2;
    uint64_t m = 0;
    for (int p = 0; p < parts; p++) {
        const size_t i = k * (size_t)parts + (size_t)p;
        int64_t u;
        if (base == SDR_DDC_SC16) {
            int16_t x;
            memcpy(&x, static_cast<const unsigned char *>(raw) + 2 * i, 2);
            u = x;
        } else if (base == SDR_DDC_CS8) {
            u = static_cast<const int8_t *>(raw)[i];
        } else {
            u = nb_unit_u8(static_cast<const uint8_t *>(raw)[i]);
        }
        m += (uint64_t)(u * u);
    }
    return m;
}

// the blank word of sample k, written over out's sample k
inline void nb_blank_word_host(void *out, int fmt, size_t k)
{
    const int sb = ddc_sample_bytes(fmt);
    unsigned char *o = static_cast<unsigned char *>(out) + k * (size_t)sb;
    if (ddc_complex_base(fmt) != SDR_DDC_CU8) {
        memset(o, 0, (size_t)sb);
        return;
    }
    o[0] = (unsigned char)(127 + (k & 1));
    if (!ddc_is_real(fmt))
        o[1] = (unsigned char)(128 - (k & 1));
}

struct NbTotals {
    int64_t impulses = 0, blanked = 0;
};

// The definition over one whole stream from k = 0: n a positive multiple of block (the caller has checked everything).
inline NbTotals nb_blank_stream_host(int fmt, int block, int window, int ratio_q4, int hold, const void *in, size_t n, void *out)
{
    const size_t B = (size_t)block, W = (size_t)window, blocks = n / B;
    memcpy(out, in, n * (size_t)ddc_sample_bytes(fmt));
    std::vector<uint64_t> P(blocks);
    for (size_t j = 0; j < blocks; j++) {
        uint64_t p = 0;
        for (size_t k = j * B; k < (j + 1) * B; k++)
            p += nb_mag_host(in, fmt, k);
        P[j] = p;
    }
    NbTotals t;
    bool open = false;
    size_t last = 0;  // the last impulse, while open
    for (size_t j = 0; j < blocks; j++) {
        uint64_t R = 0;
        for (size_t i = 1; i <= W && i <= j; i++)
            R += P[j - i];
        for (size_t k = j * B; k < (j + 1) * B; k++) {
            if (j >= W && nb_is_impulse(nb_mag_host(in, fmt, k), block * window, ratio_q4, R)) {
                t.impulses++;
                open = true;
                last = k;
            }
            if (open && k - last <= (size_t)hold) {
                nb_blank_word_host(out, fmt, k);
                t.blanked++;
            }
        }
    }
    return t;
}

}  // namespace sdr
