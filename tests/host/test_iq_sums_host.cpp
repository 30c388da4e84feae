// The host side of the raw-stream sums (sdrainer_amd/csrc/host/iq_sums.h) walked without a GPU, driven by
// tests/test_iqc_ref.py: which formats are summed and their units and scales, the unit transform against a direct sum, the
// bookkeeping of n and skipped around 2^32, and the refusals of iq_correction_from_sums.  With arguments
// "<format> n sum_i sum_q sum_ii sum_qq sum_iq" it prints the four float32 words of the correction (or "refused").
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../sdrainer_amd/csrc/host/iq_sums.h"

static int failures = 0;
#define EXPECT(c)                                              \
    do {                                                       \
        if (!(c)) {                                            \
            printf("FAILED line %d: %s\n", __LINE__, #c);      \
            failures++;                                        \
        }                                                      \
    } while (0)

static void formats()
{
    int n = 0;
    for (int f = -2; f <= 40; f++)
        n += sdr::iq_sums_format(f);
    EXPECT(n == 3 && sdr::iq_sums_format(SDR_DDC_CS8) && sdr::iq_sums_format(SDR_DDC_CU8) && sdr::iq_sums_format(SDR_DDC_SC16));
    EXPECT(!sdr::iq_sums_format(SDR_DDC_F32) && !sdr::iq_sums_format(SDR_DDC_RS8) && !sdr::iq_sums_format(SDR_DDC_RS16));
    EXPECT(sdr::iq_unit_scale(SDR_DDC_CS8) == 128.0 && sdr::iq_unit_scale(SDR_DDC_CU8) == 256.0 && sdr::iq_unit_scale(SDR_DDC_SC16) == 32767.0);
    static_assert(sizeof(sdr_iq_sums) == 64 && sizeof(sdr_iq_correction) == 16, "");
}

// the kernel sums b = byte ^ flip; the record holds u = a b + c: every byte pair against the direct sum
static void units()
{
    for (int fmt : {SDR_DDC_CS8, SDR_DDC_CU8}) {
        const sdr::IqUnit u = sdr::iq_unit(fmt);
        sdr::IqRawSums b{}, want{};
        int64_t n = 0;
        for (int x = 0; x < 256; x++)
            for (int y = 0; y < 256; y += 5) {
                // the raw bytes x, y: cs8 reads them as int8, cu8 as uint8
                const int64_t bi = fmt == SDR_DDC_CS8 ? (x ^ 0x80) : x, bq = fmt == SDR_DDC_CS8 ? (y ^ 0x80) : y;
                const int64_t ui = fmt == SDR_DDC_CS8 ? (int8_t)x : 2 * x - 255, uq = fmt == SDR_DDC_CS8 ? (int8_t)y : 2 * y - 255;
                b.i += bi, b.q += bq, b.ii += bi * bi, b.qq += bq * bq, b.iq += bi * bq;
                want.i += ui, want.q += uq, want.ii += ui * ui, want.qq += uq * uq, want.iq += ui * uq;
                n++;
            }
        const sdr::IqRawSums got = sdr::iq_unit_sums(b, u, n);
        EXPECT(got.i == want.i && got.q == want.q && got.ii == want.ii && got.qq == want.qq && got.iq == want.iq);
    }
    const sdr::IqRawSums s{-5, 7, 25, 49, -35};
    const sdr::IqRawSums same = sdr::iq_unit_sums(s, sdr::iq_unit(SDR_DDC_SC16), 1);
    EXPECT(same.i == -5 && same.q == 7 && same.ii == 25 && same.qq == 49 && same.iq == -35);
    // a whole call of the most negative word: 2^31 - 1 samples of cs8 -128 (b = 0) and of cu8 0 (b = 0)
    const int64_t big = 2147483647;
    const sdr::IqRawSums z = sdr::iq_unit_sums(sdr::IqRawSums{}, sdr::iq_unit(SDR_DDC_CS8), big);
    EXPECT(z.i == -128 * big && z.ii == 16384 * big && z.iq == 16384 * big);
    const sdr::IqRawSums w = sdr::iq_unit_sums(sdr::IqRawSums{}, sdr::iq_unit(SDR_DDC_CU8), big);
    EXPECT(w.q == -255 * big && w.qq == 65025 * big);
}

static void bookkeeping()
{
    const int64_t two32 = (int64_t)1 << 32, call = 2147483647;  // the longest call: n_in_samples is an int
    sdr::IqSumsCount c;
    EXPECT(c.n == 0 && c.skipped == 0);
    EXPECT(c.accept(call) && c.n == call && c.skipped == 0);
    EXPECT(c.accept(call) && c.n == 2 * call);
    EXPECT(c.accept(1) && c.accept(1) && c.n == two32);     // exactly 2^32 is summed
    EXPECT(!c.accept(1) && c.n == two32 && c.skipped == 1);  // one more is not
    EXPECT(!c.accept(call) && c.n == two32 && c.skipped == 1 + call);
    c.clear();
    EXPECT(c.n == 0 && c.skipped == 0 && c.accept(8) && c.n == 8);
    // a call that does not fit is skipped whole, and a shorter one behind it is still summed
    sdr::IqSumsCount d;
    d.n = two32 - 10;
    EXPECT(!d.accept(11) && d.skipped == 11 && d.n == two32 - 10);
    EXPECT(d.accept(10) && d.n == two32 && d.skipped == 11);
    // sum_ii stays within 2^62: 2^32 samples of sc16 -32768
    EXPECT(two32 * ((int64_t)32768 * 32768) == (int64_t)1 << 62);
}

static void refusals()
{
    const sdr_iq_correction mark = {1.5f, 2.5f, 3.5f, 4.5f};
    const sdr_iq_sums good = {1000, 100, -200, 5000000, 5100000, 30000, 0, 0};
    struct {
        sdr_iq_sums s;
        int fmt;
    } bad[] = {
        {good, SDR_DDC_F32}, {good, SDR_DDC_RS8}, {good, 4}, {good, -1},
        {{1, 5, 5, 25, 25, 25, 0, 0}, SDR_DDC_CS8},             // n < 2
        {{0, 0, 0, 0, 0, 0, 0, 0}, SDR_DDC_CS8},
        {{-4, 0, 0, 0, 0, 0, 0, 0}, SDR_DDC_CS8},
        {{4, 20, 0, 100, 400, 0, 0, 0}, SDR_DDC_SC16},           // I constant: vi = 0
        {{4, 0, 0, 20, 80, 40, 0, 0}, SDR_DDC_SC16},             // Q = 2 I: r = 0
        {{4, 0, 0, 20, 0, 0, 0, 0}, SDR_DDC_CU8},                // Q constant: r = 0
    };
    for (auto &b : bad) {
        sdr_iq_correction out = mark;
        EXPECT(!sdr::iq_correction_from_sums(b.s, b.fmt, &out));
        EXPECT(memcmp(&out, &mark, sizeof out) == 0);
    }
    sdr_iq_correction out = mark;
    EXPECT(sdr::iq_correction_from_sums(good, SDR_DDC_CS8, &out) && out.gain_im > 0.9f && out.gain_im < 1.1f);
}

int main(int argc, char **argv)
{
    if (argc == 8) {
        sdr_iq_sums s{};
        s.n = strtoll(argv[2], nullptr, 10), s.sum_i = strtoll(argv[3], nullptr, 10), s.sum_q = strtoll(argv[4], nullptr, 10);
        s.sum_ii = strtoll(argv[5], nullptr, 10), s.sum_qq = strtoll(argv[6], nullptr, 10), s.sum_iq = strtoll(argv[7], nullptr, 10);
        sdr_iq_correction c;
        if (!sdr::iq_correction_from_sums(s, atoi(argv[1]), &c)) {
            printf("refused\n");
            return 0;
        }
        uint32_t w[4];
        memcpy(w, &c, sizeof w);
        printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", w[0], w[1], w[2], w[3]);
        return 0;
    }
    formats();
    units();
    bookkeeping();
    refusals();
    if (!failures)
        printf("iq sums ok\n");
    return failures != 0;
}
