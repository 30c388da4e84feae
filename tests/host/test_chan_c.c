/* A PLAIN C caller of the channelizer (include/sdrainer_hip.h, sdr_chan_*): compiled with gcc -std=c11 -Wall -Werror
 * -pedantic by tests/test_chan_c.py, which also checks that every sdr_chan_* declaration is taken by address here.
 * create -> argument checks -> process_host (two calls) -> copy the streams' outputs back -> destroy, printing every output
 * as hex words, stream by stream.  Device memory comes from the HIP runtime, declared by hand as a cgo host would.
 * usage: test_chan_c <raw samples> <format> <n_channels> <decimation> <taps.f32> <n_taps> <n_samples> <channel> [<channel> ...]
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

/* every channelizer entry point, by its declared type: a declaration that changes breaks this build */
static int (*const chan_create)(const sdr_chan_config *, const float *, const int32_t *, sdr_chan **) = sdr_chan_create;
static int (*const chan_destroy)(sdr_chan *) = sdr_chan_destroy;
static int (*const chan_sync)(sdr_chan *) = sdr_chan_sync;
static int (*const chan_set_stream)(sdr_chan *, void *) = sdr_chan_set_stream;
static int (*const chan_set_first_sample)(sdr_chan *, int64_t) = sdr_chan_set_first_sample;
static int64_t (*const chan_total_samples)(sdr_chan *) = sdr_chan_total_samples;
static int (*const chan_process_device)(sdr_chan *, const void *, size_t, float *, size_t) = sdr_chan_process_device;
static int (*const chan_process_host)(sdr_chan *, const void *, size_t, float *, size_t) = sdr_chan_process_host;
static int (*const chan_tile_outputs)(int, int, int) = sdr_chan_tile_outputs;

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
    if (argc < 9) {
        fprintf(stderr, "usage: %s <raw samples> <format> <n_channels> <decimation> <taps.f32> <n_taps> <n_samples> <channel> [<channel> ...]\n", argv[0]);
        return 2;
    }
    const int format = atoi(argv[2]), m_ch = atoi(argv[3]), d = atoi(argv[4]), t = atoi(argv[6]), n = atoi(argv[7]), streams = argc - 8;
    const int base = format & ~SDR_DDC_REAL;
    const size_t value_bytes = base == SDR_DDC_F32 ? 4 : base == SDR_DDC_SC16 ? 2 : 1;
    const size_t sample_bytes = (format & SDR_DDC_REAL) ? value_bytes : 2 * value_bytes;
    int32_t channels[256];
    for (int i = 0; i < streams && i < 256; i++)
        channels[i] = atoi(argv[8 + i]);
    unsigned char *raw = read_file(argv[1], (size_t)n * sample_bytes);
    float *taps = read_file(argv[5], (size_t)t * sizeof *taps);

    if (chan_tile_outputs(m_ch, d, t) < 16 || chan_tile_outputs(m_ch + 1, d, t) >= 0 || chan_tile_outputs(m_ch, d, t + 1) >= 0) {
        fprintf(stderr, "sdr_chan_tile_outputs is off\n");
        return 1;
    }

    sdr_chan_config cfg = {0};
    cfg.struct_size = (int32_t)sizeof cfg;
    cfg.n_channels = m_ch;
    cfg.decimation = d;
    cfg.n_taps = t;
    cfg.in_format = format;
    cfg.max_in_samples = n;
    cfg.n_out = streams;
    sdr_chan *chan = NULL;
    sdr_chan_config bad = cfg;
    bad.struct_size -= 4;
    sdr_chan_config odd = cfg;
    odd.decimation = 3 * d;
    if (chan_create(&bad, taps, channels, &chan) != SDR_ERR_BAD_ARG || chan_create(&cfg, NULL, channels, &chan) != SDR_ERR_BAD_ARG ||
        chan_create(&odd, taps, channels, &chan) != SDR_ERR_BAD_ARG || chan != NULL) {
        fprintf(stderr, "sdr_chan_create took a bad argument\n");
        return 1;
    }
    CHECK(chan_create(&cfg, taps, channels, &chan));
    CHECK(chan_set_stream(chan, NULL));
    CHECK(chan_set_first_sample(chan, 0));

    const size_t m = (size_t)(n / d), stride = (m + 3) / 4 * 4;
    float *out_dev = NULL;
    if (hipMalloc((void **)&out_dev, (size_t)streams * stride * 2 * sizeof(float)) != 0) {
        fprintf(stderr, "hipMalloc failed\n");
        return 1;
    }
    /* argument checks: none of them may launch anything or move the stream on */
    if (chan_process_host(chan, raw, (size_t)n + 1, out_dev, stride) != SDR_ERR_BAD_SIZE || chan_process_host(chan, NULL, (size_t)n, out_dev, stride) != SDR_ERR_BAD_ARG ||
        chan_process_device(chan, raw, (size_t)n, out_dev + 1, stride) != SDR_ERR_BAD_ARG || chan_process_host(chan, raw, (size_t)n, out_dev, stride + 2) != SDR_ERR_BAD_ARG ||
        chan_total_samples(chan) != 0) {
        fprintf(stderr, "an argument check did not return its status\n");
        return 1;
    }
    /* two calls: the first half of the outputs, then the rest behind them */
    const size_t m0 = m / 2 / 2 * 2; /* (even: the second call's output pointer stays 16-byte aligned) */
    if (m0 > 0)
        CHECK(chan_process_host(chan, raw, m0 * (size_t)d, out_dev, stride));
    CHECK(chan_process_host(chan, raw + m0 * (size_t)d * sample_bytes, (m - m0) * (size_t)d, out_dev + 2 * m0, stride));
    CHECK(chan_sync(chan));
    if (chan_set_first_sample(chan, 0) != SDR_ERR_STATE || chan_total_samples(chan) != (int64_t)(m * (size_t)d)) {
        fprintf(stderr, "the channelizer's sample count is off\n");
        return 1;
    }
    float *out = malloc((size_t)streams * stride * 2 * sizeof *out);
    if (!out || hipMemcpy(out, out_dev, (size_t)streams * stride * 2 * sizeof *out, HIP_MEMCPY_DEVICE_TO_HOST) != 0) {
        fprintf(stderr, "hipMemcpy failed\n");
        return 1;
    }
    printf("outputs %d\n", (int)m);
    for (int b = 0; b < streams; b++) {
        printf("channel");
        for (size_t k = 0; k < 2 * m; k++) {
            union {
                float f;
                uint32_t u;
            } w = {out[(size_t)b * stride * 2 + k]};
            printf(" %08x", (unsigned)w.u);
        }
        printf("\n");
    }
    CHECK(chan_destroy(chan));
    hipFree(out_dev);
    free(out);
    free(raw);
    free(taps);
    printf("done\n");
    return 0;
}
