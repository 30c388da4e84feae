/* A PLAIN C caller of the sc16 entry points (include/sdrainer_hip.h, *_sc16): compiled with gcc -std=c11 -Wall -Werror
 * -pedantic by tests/test_sc16_c.py, which also checks that every sc16 declaration is taken by address here.
 * create -> push_iq_sc16 -> process_staged -> read_spectrum -> destroy, printing the last frame's psd as hex words.
 * usage: test_sc16_c <iq.s16> <rate> <n> <frames>   (the file holds [frame][n][2] little-endian int16)
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

/* every sc16 entry point, by its declared type: a declaration that changes breaks this build */
static int (*const push_sc16)(sdr_bank *, int, int, const int16_t *, size_t) = sdr_push_iq_sc16;
static int (*const process_sc16)(sdr_bank *, const int16_t *, int) = sdr_process_device_sc16;
static int (*const capture_sc16)(sdr_bank *, int) = sdr_graph_capture_sc16;
static int (*const launch_sc16)(sdr_bank *, const int16_t *const *) = sdr_graph_launch_sc16;
static int (*const group_push_sc16)(sdr_group *, int, int, const int16_t *, size_t) = sdr_group_push_iq_sc16;
static int (*const group_process_sc16)(sdr_group *, const int16_t *const *, int) = sdr_group_process_device_sc16;

int main(int argc, char **argv)
{
    if (argc != 5) {
        fprintf(stderr, "usage: %s <iq.s16> <rate> <n> <frames>\n", argv[0]);
        return 2;
    }
    const int rate = atoi(argv[2]), n = atoi(argv[3]), frames = atoi(argv[4]);
    const size_t values = (size_t)frames * (size_t)n * 2;
    int16_t *iq = malloc(values * sizeof *iq);
    float *psd = malloc((size_t)n * sizeof *psd);
    FILE *f = fopen(argv[1], "rb");
    if (!iq || !psd || !f || fread(iq, sizeof *iq, values, f) != values) {
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
    if (process_sc16(bank, NULL, frames) != SDR_ERR_BAD_ARG || launch_sc16(bank, NULL) != SDR_ERR_BAD_ARG ||
        capture_sc16(bank, frames + 1) != SDR_ERR_BAD_ARG || group_push_sc16(NULL, 0, rate, iq, values) != SDR_ERR_BAD_ARG ||
        group_process_sc16(NULL, NULL, frames) != SDR_ERR_BAD_ARG || push_sc16(bank, 0, rate + 1, iq, values) != SDR_ERR_BAD_RATE) {
        fprintf(stderr, "an argument check did not return its status\n");
        return 1;
    }
    CHECK(push_sc16(bank, 0, rate, iq, values));
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
