/* A PLAIN C caller of the down-converter (include/sdrainer_hip.h, sdr_ddc_*): compiled with gcc -std=c11 -Wall -Werror
 * -pedantic by tests/test_ddc_c.py, which also checks that every sdr_ddc_* declaration is taken by address here.
 * create -> argument checks -> process_host (two calls) -> copy the bands' outputs back -> destroy, printing every output as
 * hex words, band by band.  Device memory comes from the HIP runtime, declared by hand as a cgo host would.
 * usage: test_ddc_c <raw samples> <format> <decimation> <taps.f32> <n_taps> <n_samples> <step> [<step> ...]
 */
#include <stdio.h>
#include <stdlib.h>

#include "../../include/sdrainer_hip.h"

/* the three HIP runtime calls a host needs to own the output ring (hipError_t and hipMemcpyKind are ints) */
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

/* every DDC entry point, by its declared type: a declaration that changes breaks this build */
static int (*const ddc_create)(const sdr_ddc_config *, const float *, const int32_t *, sdr_ddc **) = sdr_ddc_create;
static int (*const ddc_destroy)(sdr_ddc *) = sdr_ddc_destroy;
static int (*const ddc_sync)(sdr_ddc *) = sdr_ddc_sync;
static int (*const ddc_set_stream)(sdr_ddc *, void *) = sdr_ddc_set_stream;
static int (*const ddc_set_first_sample)(sdr_ddc *, int64_t) = sdr_ddc_set_first_sample;
static int64_t (*const ddc_total_samples)(sdr_ddc *) = sdr_ddc_total_samples;
static int (*const ddc_set_nco_step)(sdr_ddc *, int, int) = sdr_ddc_set_nco_step;
static int (*const ddc_process_device)(sdr_ddc *, const void *, size_t, float *, size_t) = sdr_ddc_process_device;
static int (*const ddc_process_host)(sdr_ddc *, const void *, size_t, float *, size_t) = sdr_ddc_process_host;
static int (*const ddc_nco_table)(float *, float *) = sdr_ddc_nco_table;

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
    if (argc < 8) {
        fprintf(stderr, "usage: %s <raw samples> <format> <decimation> <taps.f32> <n_taps> <n_samples> <step> [<step> ...]\n", argv[0]);
        return 2;
    }
    const int format = atoi(argv[2]), d = atoi(argv[3]), t = atoi(argv[5]), n = atoi(argv[6]), bands = argc - 7;
    const size_t sample_bytes = format == SDR_DDC_F32 ? 8 : format == SDR_DDC_SC16 ? 4 : 2;
    int32_t steps[64];
    for (int b = 0; b < bands && b < 64; b++)
        steps[b] = atoi(argv[7 + b]);
    unsigned char *raw = read_file(argv[1], (size_t)n * sample_bytes);
    float *taps = read_file(argv[4], (size_t)t * sizeof *taps);

    static float co[SDR_DDC_NCO_SIZE], si[SDR_DDC_NCO_SIZE];
    CHECK(ddc_nco_table(co, si));
    if (co[0] != 1.0f || si[SDR_DDC_NCO_SIZE / 4] != 1.0f || co[SDR_DDC_NCO_SIZE / 2] != -1.0f || si[0] != 0.0f) {
        fprintf(stderr, "the NCO table's quarter points are off\n");
        return 1;
    }

    sdr_ddc_config cfg = {0};
    cfg.struct_size = (int32_t)sizeof cfg;
    cfg.n_bands = bands;
    cfg.decimation = d;
    cfg.n_taps = t;
    cfg.in_format = format;
    cfg.max_in_samples = n;
    sdr_ddc *ddc = NULL;
    sdr_ddc_config bad = cfg;
    bad.struct_size -= 4;
    if (ddc_create(&bad, taps, steps, &ddc) != SDR_ERR_BAD_ARG || ddc_create(&cfg, NULL, steps, &ddc) != SDR_ERR_BAD_ARG || ddc != NULL) {
        fprintf(stderr, "sdr_ddc_create took a bad argument\n");
        return 1;
    }
    CHECK(ddc_create(&cfg, taps, steps, &ddc));
    CHECK(ddc_set_stream(ddc, NULL));
    CHECK(ddc_set_first_sample(ddc, 0));

    const size_t m = (size_t)(n / d), stride = (m + 3) / 4 * 4;
    float *out_dev = NULL;
    if (hipMalloc((void **)&out_dev, (size_t)bands * stride * 2 * sizeof(float)) != 0) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    /* argument checks: none of them may launch anything or move the stream on */
    if (ddc_process_host(ddc, raw, (size_t)n + 1, out_dev, stride) != SDR_ERR_BAD_SIZE || ddc_process_host(ddc, NULL, (size_t)n, out_dev, stride) != SDR_ERR_BAD_ARG ||
        ddc_process_device(ddc, raw, (size_t)n, out_dev + 1, stride) != SDR_ERR_BAD_ARG || ddc_process_host(ddc, raw, (size_t)n, out_dev, stride + 2) != SDR_ERR_BAD_ARG ||
        ddc_set_nco_step(ddc, bands, 0) != SDR_ERR_BAD_ARG || ddc_total_samples(ddc) != 0) {
        fprintf(stderr, "an argument check did not return its status\n");
        return 1;
    }
    /* two calls: the first half of the outputs, then the rest behind them */
    const size_t m0 = m / 2 / 2 * 2; /* (even: the second call's output pointer stays 16-byte aligned) */
    if (m0 > 0)
        CHECK(ddc_process_host(ddc, raw, m0 * (size_t)d, out_dev, stride));
    CHECK(ddc_process_host(ddc, raw + m0 * (size_t)d * sample_bytes, (m - m0) * (size_t)d, out_dev + 2 * m0, stride));
    CHECK(ddc_sync(ddc));
    if (ddc_set_first_sample(ddc, 0) != SDR_ERR_STATE || ddc_total_samples(ddc) != (int64_t)(m * (size_t)d)) {
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
    CHECK(ddc_destroy(ddc));
    hipFree(out_dev);
    free(out);
    free(raw);
    free(taps);
    printf("done\n");
    return 0;
}
