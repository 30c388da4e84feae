/* A PLAIN C caller of the IQ correction (include/sdrainer_hip.h "IQ correction"): compiled with gcc -std=c11 -Wall -Werror
 * -pedantic by tests/test_iqc_c.py.  It takes the seven sdr_iq_* entry points by address with their declared types (the test
 * checks that every such declaration of the header is taken here), checks the two structs' sizes and field offsets, and calls the one entry point
 * that needs no GPU: sdr_iq_correction_from_sums, once refused (the output stays as it was) and once for a stream whose Q is
 * 1.25 times an I-independent value plus a quarter of I.
 */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "../../include/sdrainer_hip.h"

/* every entry point, by its declared type: a declaration that changes breaks this build */
static int (*const ddc_set_iq_correction)(sdr_ddc *, const sdr_iq_correction *) = sdr_iq_ddc_set_correction;
static int (*const ddc_enable_iq_sums)(sdr_ddc *, int) = sdr_iq_ddc_enable_sums;
static int (*const ddc_read_iq_sums)(sdr_ddc *, sdr_iq_sums *) = sdr_iq_ddc_read_sums;
static int (*const chan_set_iq_correction)(sdr_chan *, const sdr_iq_correction *) = sdr_iq_chan_set_correction;
static int (*const chan_enable_iq_sums)(sdr_chan *, int) = sdr_iq_chan_enable_sums;
static int (*const chan_read_iq_sums)(sdr_chan *, sdr_iq_sums *) = sdr_iq_chan_read_sums;
static int (*const correction_from_sums)(const sdr_iq_sums *, int, sdr_iq_correction *) = sdr_iq_correction_from_sums;

_Static_assert(sizeof(sdr_iq_correction) == 16, "sdr_iq_correction is 16 bytes");
_Static_assert(offsetof(sdr_iq_correction, dc_re) == 0 && offsetof(sdr_iq_correction, dc_im) == 4, "");
_Static_assert(offsetof(sdr_iq_correction, gain_im) == 8 && offsetof(sdr_iq_correction, cross) == 12, "");
_Static_assert(sizeof(sdr_iq_sums) == 64, "sdr_iq_sums is 64 bytes");
_Static_assert(offsetof(sdr_iq_sums, n) == 0 && offsetof(sdr_iq_sums, sum_i) == 8 && offsetof(sdr_iq_sums, sum_q) == 16, "");
_Static_assert(offsetof(sdr_iq_sums, sum_ii) == 24 && offsetof(sdr_iq_sums, sum_qq) == 32 && offsetof(sdr_iq_sums, sum_iq) == 40, "");
_Static_assert(offsetof(sdr_iq_sums, skipped) == 48 && offsetof(sdr_iq_sums, reserved) == 56, "");
_Static_assert(sizeof(sdr_ddc_config) == 32 && sizeof(sdr_chan_config) == 32, "the config structs stay 32 bytes");

int main(void)
{
    if (sdr_abi_version() != 2) {
        fprintf(stderr, "sdr_abi_version is not 2\n");
        return 1;
    }
    /* null handles are refused without a GPU */
    sdr_iq_sums got;
    if (ddc_set_iq_correction(NULL, NULL) != SDR_ERR_BAD_ARG || ddc_enable_iq_sums(NULL, 1) != SDR_ERR_BAD_ARG ||
        ddc_read_iq_sums(NULL, &got) != SDR_ERR_BAD_ARG || chan_set_iq_correction(NULL, NULL) != SDR_ERR_BAD_ARG ||
        chan_enable_iq_sums(NULL, 1) != SDR_ERR_BAD_ARG || chan_read_iq_sums(NULL, &got) != SDR_ERR_BAD_ARG) {
        fprintf(stderr, "a null handle was accepted\n");
        return 1;
    }
    const sdr_iq_correction mark = {1.5f, 2.5f, 3.5f, 4.5f};
    sdr_iq_correction c = mark;
    sdr_iq_sums one = {1, 3, 4, 9, 16, 12, 0, 0};
    if (correction_from_sums(&one, SDR_DDC_CS8, &c) != SDR_ERR_BAD_ARG || correction_from_sums(NULL, SDR_DDC_CS8, &c) != SDR_ERR_BAD_ARG ||
        memcmp(&c, &mark, sizeof c) != 0) {
        fprintf(stderr, "sdr_iq_correction_from_sums took bad sums or wrote its output\n");
        return 1;
    }
    /* i = (5, -3, 5, -3) = i0 + 1, q0 = (4, 4, -4, -4), q = 1.25 q0 + 0.25 i0 - 2 = (4, 2, -6, -8): the estimate undoes it exactly */
    sdr_iq_sums s = {4, 4, -8, 68, 120, 8, 0, 0};
    if (correction_from_sums(&s, SDR_DDC_CS8, &c) != SDR_OK || c.dc_re != 1.0f / 128.0f || c.dc_im != -2.0f / 128.0f || c.gain_im != 0.8f ||
        c.cross != -0.2f) {
        fprintf(stderr, "sdr_iq_correction_from_sums: %g %g %g %g\n", c.dc_re, c.dc_im, c.gain_im, c.cross);
        return 1;
    }
    printf("layout ok\n");
    return 0;
}
