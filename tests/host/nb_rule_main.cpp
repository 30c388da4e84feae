// A stand-alone walk over csrc/host/nb_rule.h, the impulse noise blanker's integer rule, without HIP and without the library:
// tests/test_nb_rule_host.py builds and runs it; built with -fsanitize=address,undefined it is also the sanitizer run of the
// host-only code (every buffer below is a heap block of exactly the stream's size).
//   1. nb_threshold / nb_over decide what nb_is_impulse decides, at the limits of every quantity and for random values;
//   2. the extreme stream (sc16 -32768 / -32768, B * W = 65536, ratio_q4 = 16384) leaves both sides below 2^52 and 2^62;
//   3. nb_blank_stream_host over every format: impulses at a block's first and last sample and at the stream's last sample,
//      hold = 0 and hold = B, and the uint8 blank words' parity.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../sdrainer_amd/csrc/host/nb_rule.h"

using namespace sdr;

static int fail(const char *what)
{
    fprintf(stderr, "nb_rule: %s\n", what);
    return 1;
}

static int thresholds()
{
    std::mt19937_64 rng(7);
    const uint64_t ms[] = {0, 1, 2, 255, 65025, 130050, 1ull << 30, (1ull << 31) - 1, 1ull << 31};
    for (int span_log2 = 6; span_log2 <= 16; span_log2++) {
        const int span = 1 << span_log2;
        const uint64_t r_max = kNbMaxM * (uint64_t)span;
        for (int ratio : {0, 16, 17, 192, 4096, 16383, 16384}) {
            for (int i = 0; i < 4000; i++) {
                const uint64_t R = i == 0 ? 0 : i == 1 ? r_max : i == 2 ? 1 : rng() % (r_max + 1) >> (rng() % 48);
                const uint32_t thr = nb_threshold(R, ratio, span_log2, true);
                for (uint64_t m : ms)
                    if (nb_over((uint32_t)m, thr) != nb_is_impulse(m, span, ratio, R))
                        return fail("nb_threshold disagrees with the inequality");
                // around the threshold itself
                for (uint64_t m = thr == kNbNever ? 0 : thr; m <= (thr == kNbNever ? 0 : (uint64_t)thr + 1) && m <= kNbMaxM; m++)
                    if (nb_over((uint32_t)m, thr) != nb_is_impulse(m, span, ratio, R))
                        return fail("nb_threshold disagrees with the inequality at the threshold");
            }
            if (nb_threshold(12345, ratio, span_log2, false) != kNbNever)
                return fail("an unjudged block has a threshold");
        }
    }
    return 0;
}

static int extremes()
{
    const int B = 4096, W = 16;
    const size_t n = (size_t)(W + 2) * B;
    int16_t *in = (int16_t *)malloc(n * 4), *out = (int16_t *)malloc(n * 4);
    for (size_t i = 0; i < 2 * n; i++)
        in[i] = -32768;
    const uint64_t m = nb_mag_host(in, SDR_DDC_SC16, n - 1);
    const uint64_t left = m * (uint64_t)(B * W) * 16u, right = 16384ull * (m * (uint64_t)(B * W));
    int rc = 0;
    if (m != kNbMaxM || left >= (1ull << 52) || right >= (1ull << 62) || left / 16 / (B * W) != m || right / 16384 / m != (uint64_t)(B * W))
        rc = fail("the extreme values wrap");
    for (int ratio : {16, 16384}) {  // 16: both sides are equal, and "greater" decides
        const NbTotals t = nb_blank_stream_host(SDR_DDC_SC16, B, W, ratio, 3, in, n, out);
        if (t.impulses != 0 || t.blanked != 0 || memcmp(in, out, n * 4) != 0)
            rc = fail("a constant extreme stream has an impulse");
    }
    free(in);
    free(out);
    return rc;
}

static int streams()
{
    const int fmts[] = {SDR_DDC_SC16, SDR_DDC_CS8, SDR_DDC_CU8, SDR_DDC_RS16, SDR_DDC_RS8, SDR_DDC_RU8};
    const int B = 64, W = 2;
    const size_t n = 6 * (size_t)B;
    for (int fmt : fmts) {
        if (!nb_format(fmt))
            return fail("a format is refused");
        const size_t sb = (size_t)ddc_sample_bytes(fmt);
        const bool u8 = ddc_complex_base(fmt) == SDR_DDC_CU8;
        for (int hold : {0, 3, B}) {
            unsigned char *in = (unsigned char *)malloc(n * sb), *out = (unsigned char *)malloc(n * sb);
            memset(in, u8 ? 128 : 0, n * sb);  // u = 1 or 0 throughout
            const size_t places[] = {(size_t)B - 1, 3 * (size_t)B, 4 * (size_t)B - 1, n - 1};  // the first one is not judged
            for (size_t p : places)
                memset(in + p * sb, u8 ? 255 : 0x80, sb);  // sc16 0x8080 = -32640
            const NbTotals t = nb_blank_stream_host(fmt, B, W, 64, hold, in, n, out);
            long long want = 0;
            int rc = 0;
            for (size_t k = 0; k < n; k++) {
                const bool blank = (k >= places[1] && k <= places[1] + (size_t)hold) || (k >= places[2] && k <= places[2] + (size_t)hold) || k == n - 1;
                want += blank;
                for (size_t b = 0; b < sb; b++) {
                    const unsigned char word = !u8 ? 0 : (unsigned char)(b == 0 ? 127 + (k & 1) : 128 - (k & 1));
                    if (out[k * sb + b] != (blank ? word : in[k * sb + b]))
                        rc = fail("a sample of a blanked stream");
                }
            }
            if (t.impulses != 3 || t.blanked != want)
                rc = fail("the totals of a blanked stream");
            free(in);
            free(out);
            if (rc)
                return rc;
        }
    }
    if (nb_format(SDR_DDC_F32) || nb_format(SDR_DDC_RF32) || nb_format(4) || nb_geometry(32, 1) || nb_geometry(4096, 32) || nb_geometry(96, 2) ||
        !nb_geometry(4096, 16) || !nb_geometry(64, 64) || nb_threshold_valid(64, 15, 0) || nb_threshold_valid(64, 16, 65) || !nb_threshold_valid(64, 0, 64))
        return fail("the limits");
    return 0;
}

int main()
{
    if (thresholds() || extremes() || streams())
        return 1;
    printf("nb rule ok\n");
    return 0;
}
