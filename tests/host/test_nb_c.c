/* A PLAIN C caller of the impulse noise blanker (include/sdrainer_hip.h "impulse noise blanker"): compiled with gcc -std=c11
 * -Wall -Werror -pedantic by tests/test_nb_c.py.  It takes the twelve sdr_nb_* entry points by address with their declared
 * types (the test checks that every such declaration of the header is taken here), checks the two structs' sizes and field
 * offsets, sees null handles refused, and calls the entry points that need no GPU: sdr_nb_tile_samples, and
 * sdr_nb_blank_host on a 128-sample cs8 stream with one planted impulse.
 */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "../../include/sdrainer_hip.h"

/* every entry point, by its declared type: a declaration that changes breaks this build */
static int (*const nb_create)(const sdr_nb_config *, sdr_nb **) = sdr_nb_create;
static int (*const nb_destroy)(sdr_nb *) = sdr_nb_destroy;
static int (*const nb_sync)(sdr_nb *) = sdr_nb_sync;
static int (*const nb_set_stream)(sdr_nb *, void *) = sdr_nb_set_stream;
static int (*const nb_set_first_sample)(sdr_nb *, int64_t) = sdr_nb_set_first_sample;
static int64_t (*const nb_total_samples)(sdr_nb *) = sdr_nb_total_samples;
static int (*const nb_set_threshold)(sdr_nb *, int, int) = sdr_nb_set_threshold;
static int (*const nb_process_device)(sdr_nb *, const void *, size_t, void *) = sdr_nb_process_device;
static int (*const nb_process_host)(sdr_nb *, const void *, size_t, void *) = sdr_nb_process_host;
static int (*const nb_read_stats)(sdr_nb *, sdr_nb_stats *) = sdr_nb_read_stats;
static int (*const nb_tile_samples)(int, int) = sdr_nb_tile_samples;
static int (*const nb_blank_host)(const sdr_nb_config *, const void *, size_t, void *, sdr_nb_stats *) = sdr_nb_blank_host;

_Static_assert(sizeof(sdr_nb_config) == 32, "sdr_nb_config is 32 bytes");
_Static_assert(offsetof(sdr_nb_config, struct_size) == 0 && offsetof(sdr_nb_config, in_format) == 4, "");
_Static_assert(offsetof(sdr_nb_config, block) == 8 && offsetof(sdr_nb_config, window) == 12, "");
_Static_assert(offsetof(sdr_nb_config, ratio_q4) == 16 && offsetof(sdr_nb_config, hold) == 20, "");
_Static_assert(offsetof(sdr_nb_config, max_in_samples) == 24 && offsetof(sdr_nb_config, device_id) == 28, "");
_Static_assert(sizeof(sdr_nb_stats) == 32, "sdr_nb_stats is 32 bytes");
_Static_assert(offsetof(sdr_nb_stats, samples) == 0 && offsetof(sdr_nb_stats, impulses) == 8, "");
_Static_assert(offsetof(sdr_nb_stats, blanked) == 16 && offsetof(sdr_nb_stats, reserved) == 24, "");
_Static_assert(sizeof(sdr_ddc_config) == 32 && sizeof(sdr_chan_config) == 32, "the other config structs stay 32 bytes");

int main(void)
{
    if (sdr_abi_version() != 2) {
        fprintf(stderr, "sdr_abi_version is not 2\n");
        return 1;
    }
    /* null handles are refused without a GPU */
    sdr_nb_stats st;
    signed char in[128][2], out[128][2];
    if (nb_sync(NULL) != SDR_ERR_BAD_ARG || nb_set_stream(NULL, NULL) != SDR_ERR_BAD_ARG || nb_set_first_sample(NULL, 0) != SDR_ERR_BAD_ARG ||
        nb_total_samples(NULL) != 0 || nb_set_threshold(NULL, 64, 3) != SDR_ERR_BAD_ARG ||
        nb_process_device(NULL, in, 64, out) != SDR_ERR_BAD_ARG || nb_process_host(NULL, in, 64, out) != SDR_ERR_BAD_ARG ||
        nb_read_stats(NULL, &st) != SDR_ERR_BAD_ARG || nb_destroy(NULL) != SDR_OK) {
        fprintf(stderr, "a null handle was accepted\n");
        return 1;
    }
    sdr_nb_config cfg = {sizeof(sdr_nb_config), SDR_DDC_F32, 64, 1, 64, 2, 64, 0};
    sdr_nb *nb = NULL;
    if (nb_create(NULL, &nb) != SDR_ERR_BAD_ARG || nb_create(&cfg, NULL) != SDR_ERR_BAD_ARG || nb_create(&cfg, &nb) != SDR_ERR_BAD_ARG || nb) {
        fprintf(stderr, "sdr_nb_create took a null pointer or a float32 format\n");
        return 1;
    }
    if (nb_tile_samples(SDR_DDC_CS8, 64) != 8192 || nb_tile_samples(SDR_DDC_SC16, 4096) != 4096 || nb_tile_samples(SDR_DDC_RU8, 64) != 16384 ||
        nb_tile_samples(SDR_DDC_F32, 64) >= 0 || nb_tile_samples(SDR_DDC_CS8, 48) >= 0) {
        fprintf(stderr, "sdr_nb_tile_samples\n");
        return 1;
    }
    /* 128 cs8 samples of (1, -1), B = 64, W = 1: block 1 is judged against P[0] = 128.  Sample 70 = (-128, 127) is an
     * impulse (m = 32513; 32513 * 64 * 16 > 64 * 128), hold = 2 blanks samples 70 .. 72; sample 5 = (100, 100) lies in
     * the block that is not judged. */
    for (int k = 0; k < 128; k++) {
        in[k][0] = 1;
        in[k][1] = -1;
    }
    in[5][0] = in[5][1] = 100;
    in[70][0] = -128;
    in[70][1] = 127;
    memset(out, 0x55, sizeof out);
    cfg.in_format = SDR_DDC_CS8;
    if (nb_blank_host(&cfg, in, 100, out, &st) != SDR_ERR_BAD_SIZE || nb_blank_host(&cfg, NULL, 128, out, &st) != SDR_ERR_BAD_ARG ||
        nb_blank_host(&cfg, in, 128, in, &st) != SDR_ERR_BAD_ARG || out[0][0] != 0x55) {
        fprintf(stderr, "sdr_nb_blank_host took a bad call or wrote its output\n");
        return 1;
    }
    if (nb_blank_host(&cfg, in, 128, out, &st) != SDR_OK || st.samples != 128 || st.impulses != 1 || st.blanked != 3 || st.reserved != 0) {
        fprintf(stderr, "sdr_nb_blank_host: %lld %lld %lld\n", (long long)st.samples, (long long)st.impulses, (long long)st.blanked);
        return 1;
    }
    for (int k = 0; k < 128; k++) {
        const int blank = k >= 70 && k <= 72;
        if (out[k][0] != (blank ? 0 : in[k][0]) || out[k][1] != (blank ? 0 : in[k][1])) {
            fprintf(stderr, "sdr_nb_blank_host: sample %d is (%d, %d)\n", k, out[k][0], out[k][1]);
            return 1;
        }
    }
    printf("layout ok\n");
    return 0;
}
