// The down-converter's format table (sdrainer_amd/csrc/host/ddc_format.h) walked on the host over every int in [-2, 40] and
// a few far ones: which are formats, which are real, the complex base and the bytes of one sample - against the list written
// out here from include/sdrainer_hip.h.  Built by tests/test_ddc_format.py with -Wall -Wextra -Werror, plain and under
// -fsanitize=address,undefined.
#include <climits>
#include <cstdio>

#include "../../sdrainer_amd/csrc/host/ddc_format.h"

namespace {

struct Row {
    int fmt, bytes, real, base;
};
// every format there is: id, bytes per sample, real flag, complex format of the same sample type
const Row kRows[] = {
    {SDR_DDC_F32, 8, 0, SDR_DDC_F32},  {SDR_DDC_SC16, 4, 0, SDR_DDC_SC16}, {SDR_DDC_CS8, 2, 0, SDR_DDC_CS8}, {SDR_DDC_CU8, 2, 0, SDR_DDC_CU8},
    {SDR_DDC_RF32, 4, 1, SDR_DDC_F32}, {SDR_DDC_RS16, 2, 1, SDR_DDC_SC16}, {SDR_DDC_RS8, 1, 1, SDR_DDC_CS8}, {SDR_DDC_RU8, 1, 1, SDR_DDC_CU8},
};
const int kIds[] = {0, 1, 2, 3, 16, 17, 18, 19};

int failures = 0;
void expect(bool ok, const char *what, int fmt)
{
    if (!ok) {
        std::printf("FAILED %s at %d\n", what, fmt);
        failures++;
    }
}

const Row *row_of(int fmt)
{
    for (const Row &r : kRows)
        if (r.fmt == fmt)
            return &r;
    return nullptr;
}

void walk(int fmt)
{
    const Row *r = row_of(fmt);
    expect(sdr::ddc_format_valid(fmt) == (r != nullptr), "ddc_format_valid", fmt);
    if (!r)
        return;
    expect(sdr::ddc_sample_bytes(fmt) == r->bytes, "ddc_sample_bytes", fmt);
    expect(sdr::ddc_is_real(fmt) == (r->real != 0), "ddc_is_real", fmt);
    expect(sdr::ddc_complex_base(fmt) == r->base, "ddc_complex_base", fmt);
    expect(sdr::ddc_format_valid(r->base) && !sdr::ddc_is_real(r->base), "the base is a complex format", fmt);
    // a real sample is one of its complex format's two values
    expect(2 * sdr::ddc_sample_bytes(fmt | SDR_DDC_REAL) == sdr::ddc_sample_bytes(fmt & ~SDR_DDC_REAL), "a real sample is half a complex one", fmt);
}

// the table is usable in constant expressions
static_assert(sdr::ddc_format_valid(SDR_DDC_RU8) && !sdr::ddc_format_valid(4) && !sdr::ddc_format_valid(-1), "");
static_assert(sdr::ddc_sample_bytes(SDR_DDC_RS16) == 2 && sdr::ddc_is_real(SDR_DDC_RF32) && sdr::ddc_complex_base(SDR_DDC_RS8) == SDR_DDC_CS8, "");

}  // namespace

int main()
{
    for (int i = 0; i < 8; i++)
        expect(kRows[i].fmt == kIds[i], "the header's ids", kIds[i]);
    int valid = 0;
    for (int fmt = -2; fmt <= 40; fmt++) {
        walk(fmt);
        valid += sdr::ddc_format_valid(fmt);
    }
    expect(valid == 8, "eight formats in [-2, 40]", valid);
    const int far[] = {-16, -17, 48, 64, 256, 1 << 16, (1 << 16) | 17, INT_MAX, INT_MIN, INT_MIN | 17};
    for (int fmt : far)
        walk(fmt);
    std::printf("formats %s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
