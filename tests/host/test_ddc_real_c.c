/* A PLAIN C caller of the down-converter's real input (include/sdrainer_hip.h, SDR_DDC_RS16): compiled with gcc -std=c11
 * -Wall -Werror -pedantic by tests/test_ddc_real_c.py.  One int16 value per sample, as a direct-sampling receiver's ADC
 * delivers it: create -> argument checks -> process_host (two calls) -> copy the bands' outputs back -> destroy, printing
 * every output as hex words, band by band.  Device memory comes from the HIP runtime, declared by hand as a cgo host would.
 * usage: test_ddc_real_c <raw int16 samples> <decimation> <taps.f32> <n_taps> <n_samples> <step> [<step> ...]
 */
#include <stdio.h>
#include <stdlib.h>

#include "../../include/sdrainer_hip.h"

int hipMalloc(void **ptr, size_t size);
int hipMemcpy(void *dst, const void *src, size_t size, int kind);
int hipFree(void *ptr);
#define HIP_MEMCPY_DEVICE_TO_HOST 2

#define CHECK(call)                                                          \
    do {                                                                     \
        const int rc_ = (call);                                              \
        if (rc_ != SDR_OK) {                                                 \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, sdr_last_error()); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

/* the real formats are the flag with a sample type: constant expressions of the header alone */
_Static_assert(SDR_DDC_REAL == 16 && SDR_DDC_RF32 == (SDR_DDC_REAL | SDR_DDC_F32) && SDR_DDC_RS16 == (SDR_DDC_REAL | SDR_DDC_SC16), "real formats");
_Static_assert(SDR_DDC_RS8 == (SDR_DDC_REAL | SDR_DDC_CS8) && SDR_DDC_RU8 == (SDR_DDC_REAL | SDR_DDC_CU8), "real formats");
_Static_assert(sizeof(sdr_ddc_config) == 32, "sdr_ddc_config stays 32 bytes");

static void *read_file(const char *path, size_t bytes)
{
    void *p = malloc(bytes ? bytes : 1);
    FILE *f = fopen(path, "rb");
    if (!p || !f || fread(p, 1, bytes, f) != bytes) {
        fprintf(stderr, "cannot read %s\n", path);
        exit(1);
    }
    fclose(f);
    return p;
}

int main(int argc, char **argv)
{
    if (argc < 7) {
        fprintf(stderr, "usage: %s <raw int16 samples> <decimation> <taps.f32> <n_taps> <n_samples> <step> [<step> ...]\n", argv[0]);
        return 2;
    }
    const int d = atoi(argv[2]), t = atoi(argv[4]), n = atoi(argv[5]), bands = argc - 6;
    int32_t steps[64];
    for (int b = 0; b < bands && b < 64; b++)
        steps[b] = atoi(argv[6 + b]);
    int16_t *raw = read_file(argv[1], (size_t)n * sizeof *raw); /* one value per sample */
    float *taps = read_file(argv[3], (size_t)t * sizeof *taps);

    sdr_ddc_config cfg = {0};
    cfg.struct_size = (int32_t)sizeof cfg;
    cfg.n_bands = bands;
    cfg.decimation = d;
    cfg.n_taps = t;
    cfg.in_format = SDR_DDC_RS16;
    cfg.max_in_samples = n;
    sdr_ddc *ddc = NULL;
    sdr_ddc_config bad = cfg;
    bad.in_format = SDR_DDC_REAL | 4; /* the flag with no sample type behind it */
    if (sdr_ddc_create(&bad, taps, steps, &ddc) != SDR_ERR_BAD_ARG || ddc != NULL) {
        fprintf(stderr, "sdr_ddc_create took format %d\n", (int)bad.in_format);
        return 1;
    }
    CHECK(sdr_ddc_create(&cfg, taps, steps, &ddc));
    CHECK(sdr_ddc_set_stream(ddc, NULL));

    const size_t m = (size_t)(n / d), stride = (m + 3) / 4 * 4;
    float *out_dev = NULL;
    if (hipMalloc((void **)&out_dev, (size_t)bands * stride * 2 * sizeof(float)) != 0) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    /* argument checks: none of them may launch anything or move the stream on */
    if (sdr_ddc_process_host(ddc, raw, (size_t)n + 1, out_dev, stride) != SDR_ERR_BAD_SIZE || sdr_ddc_process_host(ddc, NULL, (size_t)n, out_dev, stride) != SDR_ERR_BAD_ARG ||
        sdr_ddc_process_device(ddc, out_dev + 1, (size_t)n, out_dev, stride) != SDR_ERR_BAD_ARG || sdr_ddc_total_samples(ddc) != 0) {
        fprintf(stderr, "an argument check did not return its status\n");
        return 1;
    }
    /* two calls: the first half of the outputs, then the rest behind them */
    const size_t m0 = m / 2 / 2 * 2; /* (even: the second call's output pointer stays 16-byte aligned) */
    if (m0 > 0)
        CHECK(sdr_ddc_process_host(ddc, raw, m0 * (size_t)d, out_dev, stride));
    CHECK(sdr_ddc_process_host(ddc, raw + m0 * (size_t)d, (m - m0) * (size_t)d, out_dev + 2 * m0, stride));
    CHECK(sdr_ddc_sync(ddc));
    if (sdr_ddc_total_samples(ddc) != (int64_t)(m * (size_t)d)) {
        fprintf(stderr, "the DDC's sample count is off\n");
        return 1;
    }
    float *out = malloc((size_t)bands * stride * 2 * sizeof *out);
    if (!out || hipMemcpy(out, out_dev, (size_t)bands * stride * 2 * sizeof *out, HIP_MEMCPY_DEVICE_TO_HOST) != 0) {
        fprintf(stderr, "hipMemcpy failed\n");
        return 1;
    }
    printf("outputs %d\n", (int)m);
    for (int b = 0; b < bands; b++) {
        printf("band");
        for (size_t k = 0; k < 2 * m; k++) {
            union {
                float f;
                uint32_t u;
            } w = {out[(size_t)b * stride * 2 + k]};
            printf(" %08x", (unsigned)w.u);
        }
        printf("\n");
    }
    CHECK(sdr_ddc_destroy(ddc));
    hipFree(out_dev);
    free(out);
    free(raw);
    free(taps);
    printf("done\n");
    return 0;
}
