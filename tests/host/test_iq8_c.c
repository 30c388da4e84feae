/* A PLAIN C caller of the 8-bit entry points (include/sdrainer_hip.h, *_iq8): compiled with gcc -std=c11 -Wall -Werror
 * -pedantic by tests/test_iq8_c.py, which also checks that every 8-bit declaration is taken by address here.
 * create -> argument checks -> push_iq8 -> process_staged -> read_spectrum -> destroy, printing the last frame's psd as hex
 * words.
 * usage: test_iq8_c <iq.u8> <rate> <n> <frames> <format>   (the file holds [frame][n][2] bytes; format 0 cs8, 1 cu8)
 */
#include <stdio.h>
#include <stdlib.h>

#include "../../include/sdrainer_hip.h"

#define CHECK(call)                                                          \
    do {                                                                     \
        const int rc_ = (call);                                              \
        if (rc_ != SDR_OK) {                                                 \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, sdr_last_error()); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

/* every 8-bit entry point, by its declared type: a declaration that changes breaks this build */
static int (*const push8)(sdr_bank *, int, int, const void *, size_t, int) = sdr_push_iq8;
static int (*const process8)(sdr_bank *, const void *, int, int) = sdr_process_device_iq8;
static int (*const stream8)(sdr_bank *, const void *, int, size_t, int) = sdr_process_device_stream_iq8;
static int (*const capture8)(sdr_bank *, int, int) = sdr_graph_capture_iq8;
static int (*const launch8)(sdr_bank *, const void *const *, int) = sdr_graph_launch_iq8;
static int (*const group_push8)(sdr_group *, int, int, const void *, size_t, int) = sdr_group_push_iq8;
static int (*const group_process8)(sdr_group *, const void *const *, int, int) = sdr_group_process_device_iq8;

int main(int argc, char **argv)
{
    if (argc != 6) {
        fprintf(stderr, "usage: %s <iq.u8> <rate> <n> <frames> <format>\n", argv[0]);
        return 2;
    }
    const int rate = atoi(argv[2]), n = atoi(argv[3]), frames = atoi(argv[4]), format = atoi(argv[5]);
    const size_t values = (size_t)frames * (size_t)n * 2;
    unsigned char *iq = malloc(values);
    float *psd = malloc((size_t)n * sizeof *psd);
    FILE *f = fopen(argv[1], "rb");
    if (!iq || !psd || !f || fread(iq, 1, values, f) != values) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 1;
    }
    fclose(f);
    sdr_config cfg = {0};
    cfg.struct_size = (int32_t)sizeof cfg;
    cfg.n_bands = 1;
    cfg.sample_rate = rate;
    cfg.block_size = n;
    cfg.edge_width = 70 * n / 512;
    cfg.peak_threshold = 15.0f;
    cfg.signal_debounce = 1;
    cfg.max_listeners = 4;
    cfg.max_batch_frames = frames;
    cfg.max_peaks = 256;
    cfg.find_peaks = 1;
    sdr_bank *bank = NULL;
    CHECK(sdr_create(&cfg, &bank));
    /* argument checks first: none of them may launch anything */
    const void *const none[4] = {NULL, NULL, NULL, NULL};
    if (process8(bank, NULL, frames, format) != SDR_ERR_BAD_ARG || process8(bank, iq, frames, 2) != SDR_ERR_BAD_ARG ||
        process8(bank, iq, frames, -1) != SDR_ERR_BAD_ARG || stream8(bank, NULL, frames, (size_t)frames * (size_t)n, format) != SDR_ERR_BAD_ARG ||
        stream8(bank, iq, frames, (size_t)frames * (size_t)n, 2) != SDR_ERR_BAD_ARG || launch8(bank, NULL, format) != SDR_ERR_BAD_ARG ||
        launch8(bank, none, 2) != SDR_ERR_BAD_ARG || launch8(bank, none, format) != SDR_ERR_STATE ||
        capture8(bank, frames + 1, format) != SDR_ERR_BAD_ARG || capture8(bank, frames, 2) != SDR_ERR_BAD_ARG ||
        group_push8(NULL, 0, rate, iq, values, format) != SDR_ERR_BAD_ARG || group_process8(NULL, NULL, frames, format) != SDR_ERR_BAD_ARG ||
        group_process8(NULL, none, frames, -1) != SDR_ERR_BAD_ARG || push8(bank, 0, rate + 1, iq, values, format) != SDR_ERR_BAD_RATE ||
        push8(bank, 0, rate, iq, values, 2) != SDR_ERR_BAD_ARG || push8(bank, 0, rate, iq, values, -1) != SDR_ERR_BAD_ARG ||
        push8(bank, 0, rate, NULL, values, format) != SDR_ERR_BAD_ARG || push8(bank, 0, rate, iq, values - 2, format) != SDR_ERR_BAD_SIZE) {
        fprintf(stderr, "an argument check did not return its status\n");
        return 1;
    }
    CHECK(push8(bank, 0, rate, iq, values, format));
    int done = 0;
    CHECK(sdr_process_staged(bank, &done));
    CHECK(sdr_sync(bank));
    CHECK(sdr_read_spectrum(bank, 0, frames - 1, NULL, psd));
    printf("frames %d\npsd", done);
    for (int k = 0; k < n; k++) {
        union {
            float f;
            uint32_t u;
        } w = {psd[k]};
        printf(" %08x", (unsigned)w.u);
    }
    printf("\n");
    CHECK(sdr_destroy(bank));
    free(iq);
    free(psd);
    printf("done\n");
    return 0;
}
