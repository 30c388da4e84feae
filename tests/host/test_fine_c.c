/* A PLAIN C caller of the fine converter (include/sdrainer_hip.h "fine converter"): compiled with gcc -std=c11 -Wall -Werror
 * -pedantic by tests/test_fine_c.py.  It takes the ten sdr_fine_* entry points by address with their declared types (the test
 * checks that every such declaration of the header is taken here), checks the config struct's size and field offsets, sees
 * null handles and null pointers refused, and prints what sdr_fine_tune, which needs no GPU, makes of a few targets: one line
 * "tune M D target status channel step" each, which the test compares with the integer definition.
 */
#include <stddef.h>
#include <stdio.h>

#include "../../include/sdrainer_hip.h"

/* every entry point, by its declared type: a declaration that changes breaks this build */
static int (*const fine_create)(const sdr_fine_config *, const float *, const int32_t *, const int32_t *, sdr_fine **) = sdr_fine_create;
static int (*const fine_destroy)(sdr_fine *) = sdr_fine_destroy;
static int (*const fine_sync)(sdr_fine *) = sdr_fine_sync;
static int (*const fine_set_stream)(sdr_fine *, void *) = sdr_fine_set_stream;
static int (*const fine_set_first_sample)(sdr_fine *, int64_t) = sdr_fine_set_first_sample;
static int64_t (*const fine_total_samples)(sdr_fine *) = sdr_fine_total_samples;
static int (*const fine_set_nco_step)(sdr_fine *, int, int) = sdr_fine_set_nco_step;
static int (*const fine_set_input)(sdr_fine *, int, int) = sdr_fine_set_input;
static int (*const fine_process_device)(sdr_fine *, const float *, size_t, size_t, float *, size_t) = sdr_fine_process_device;
static int (*const fine_tune)(int, int, int64_t, int32_t *, int32_t *) = sdr_fine_tune;

_Static_assert(sizeof(sdr_fine_config) == 32, "sdr_fine_config is 32 bytes");
_Static_assert(offsetof(sdr_fine_config, struct_size) == 0 && offsetof(sdr_fine_config, n_bands) == 4, "");
_Static_assert(offsetof(sdr_fine_config, n_inputs) == 8 && offsetof(sdr_fine_config, decimation) == 12, "");
_Static_assert(offsetof(sdr_fine_config, n_taps) == 16 && offsetof(sdr_fine_config, max_in_samples) == 20, "");
_Static_assert(offsetof(sdr_fine_config, device_id) == 24 && offsetof(sdr_fine_config, reserved) == 28, "");
_Static_assert(sizeof(sdr_ddc_config) == 32 && sizeof(sdr_chan_config) == 32 && sizeof(sdr_nb_config) == 32,
               "the other config structs stay 32 bytes");

int main(void)
{
    if (sdr_abi_version() != 2) {
        fprintf(stderr, "sdr_abi_version is not 2\n");
        return 1;
    }
    /* null handles are refused without a GPU */
    float io[8] = {0};
    if (fine_sync(NULL) != SDR_ERR_BAD_ARG || fine_set_stream(NULL, NULL) != SDR_ERR_BAD_ARG ||
        fine_set_first_sample(NULL, 0) != SDR_ERR_BAD_ARG || fine_total_samples(NULL) != 0 ||
        fine_set_nco_step(NULL, 0, 0) != SDR_ERR_BAD_ARG || fine_set_input(NULL, 0, 0) != SDR_ERR_BAD_ARG ||
        fine_process_device(NULL, io, 4, 4, io, 4) != SDR_ERR_BAD_ARG || fine_destroy(NULL) != SDR_OK) {
        fprintf(stderr, "a null handle was accepted\n");
        return 1;
    }
    /* and so is a bad configuration, before any device is touched */
    sdr_fine_config cfg = {sizeof(sdr_fine_config), 2, 1, 4, 8, 64, 0, 0};
    const float taps[8] = {1, 0, 0, 0, 0, 0, 0, 0};
    const int32_t steps[2] = {5, -5}, inputs[2] = {0, 1};
    sdr_fine *f = NULL;
    if (fine_create(NULL, taps, steps, NULL, &f) != SDR_ERR_BAD_ARG || fine_create(&cfg, NULL, steps, NULL, &f) != SDR_ERR_BAD_ARG ||
        fine_create(&cfg, taps, NULL, NULL, &f) != SDR_ERR_BAD_ARG || fine_create(&cfg, taps, steps, NULL, NULL) != SDR_ERR_BAD_ARG ||
        fine_create(&cfg, taps, steps, NULL, &f) != SDR_ERR_BAD_ARG ||   /* two bands, one input, no map */
        fine_create(&cfg, taps, steps, inputs, &f) != SDR_ERR_BAD_ARG || /* input 1 of one */
        f) {
        fprintf(stderr, "sdr_fine_create took a null pointer or a bad map\n");
        return 1;
    }
    static const struct {
        int m, d;
        long long target;
    } t[] = {{8, 4, 37568}, {8, 4, -71936}, {8, 4, 16384}, {8, 4, 49152}, {8, 4, -131072}, {8, 8, 32768}, {8, 8, -32768},
             {64, 32, 234567}, {256, 64, -2097152}, {8, 4, 131073}, {8, 3, 0}, {6, 3, 0}, {512, 128, 0}};
    for (size_t i = 0; i < sizeof t / sizeof t[0]; i++) {
        int32_t ch = -7, st = -9;
        const int rc = fine_tune(t[i].m, t[i].d, (int64_t)t[i].target, &ch, &st);
        printf("tune %d %d %lld %d %d %d\n", t[i].m, t[i].d, t[i].target, rc, (int)ch, (int)st);
    }
    int32_t v = 3;
    if (fine_tune(8, 4, 0, NULL, &v) != SDR_ERR_BAD_ARG || fine_tune(8, 4, 0, &v, NULL) != SDR_ERR_BAD_ARG || v != 3) {
        fprintf(stderr, "sdr_fine_tune took a null output\n");
        return 1;
    }
    printf("layout ok\n");
    return 0;
}
