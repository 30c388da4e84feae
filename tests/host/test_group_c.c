/* A PLAIN C caller of the group entry points (include/sdrainer_hip.h, sdr_group_*): what the C half of a cgo shim that
 * spreads bands over several GPUs sees.  Compiled with gcc -std=c11 -Wall -Werror -pedantic by tests/test_group_c.py.
 * create -> push_iq -> process_staged -> attach (through sdr_group_member) -> push / process -> poll -> destroy,
 * printing every keying edge and rune it gets; the Python test compares them with the oracle's.
 * usage: test_group_c <iq.f32> <rate> <n> <frames> <edge> <n_bands> <n_members> <device ...> -- <bin> [<bin> ...]
 *        the file holds [band][frame][n][2] float32; every listed bin is attached on every band behind the first 100
 *        frames, as a strainer that has just found them
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/sdrainer_hip.h"

#define CHECK(call)                                                          \
    do {                                                                     \
        const int rc_ = (call);                                              \
        if (rc_ != SDR_OK) {                                                 \
            fprintf(stderr, "%s -> %d: %s\n", #call, rc_, sdr_last_error()); \
            return 1;                                                        \
        }                                                                    \
    } while (0)

enum { MAX_CHUNKS = 256, MAX_PEAKS = 8192, MAX_LISTENERS = 256, MAX_EDGES = 65536, MAX_RUNES = 65536, MAX_BINS = 32 };

static int deliver(sdr_group *group)
{
    static sdr_chunk_result chunks[MAX_CHUNKS];
    static sdr_peak peaks[MAX_PEAKS];
    static sdr_listener_result listeners[MAX_LISTENERS];
    static sdr_edge edges[MAX_EDGES];
    static uint32_t runes[MAX_RUNES], rune_frames[MAX_RUNES];
    sdr_results r;
    memset(&r, 0, sizeof r);
    r.struct_size = (int32_t)sizeof r;
    r.chunks = chunks;
    r.chunks_cap = MAX_CHUNKS;
    r.peaks = peaks;
    r.peaks_cap = MAX_PEAKS;
    r.listeners = listeners;
    r.listeners_cap = MAX_LISTENERS;
    r.edges = edges;
    r.edges_cap = MAX_EDGES;
    r.runes = runes;
    r.rune_frames = rune_frames;
    r.runes_cap = MAX_RUNES;
    CHECK(sdr_group_poll(group, &r, 1));
    printf("batch %lld first_frame %lld frames %d\n", (long long)r.batch_index, (long long)r.first_frame, (int)r.n_frames);
    for (int c = 0; c < r.n_chunks; c++)
        printf("chunk band %d frame %lld peaks %d\n", (int)chunks[c].band, (long long)chunks[c].frame, (int)chunks[c].n_peaks);
    for (int l = 0; l < r.n_listeners; l++) {
        const sdr_listener_result *x = &listeners[l];
        printf("listener %d %d edges", (int)x->band, (int)x->listener);
        for (int e = 0; e < x->n_edges; e++)
            printf(" %u:%u", (unsigned)edges[x->first_edge + e].frame, (unsigned)edges[x->first_edge + e].state);
        printf("\nlistener %d %d runes", (int)x->band, (int)x->listener);
        for (int k = 0; k < x->n_runes; k++)
            printf(" %u", (unsigned)runes[x->first_rune + k]);
        printf("\n");
    }
    printf("dropped %llu %llu\n", (unsigned long long)r.runes_dropped, (unsigned long long)r.edges_dropped);
    return 0;
}

static int push_all(sdr_group *group, const float *iq, int n_bands, int rate, int n, int frames, int from, int count)
{
    for (int b = 0; b < n_bands; b++) {
        const float *src = iq + ((size_t)b * (size_t)frames + (size_t)from) * (size_t)n * 2u;
        CHECK(sdr_group_push_iq(group, b, rate, src, (size_t)count * (size_t)n * 2u));
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 10) {
        fprintf(stderr, "usage: %s <iq.f32> <rate> <n> <frames> <edge> <n_bands> <n_members> <device ...> -- <bin> ...\n", argv[0]);
        return 2;
    }
    const int rate = atoi(argv[2]), n = atoi(argv[3]), frames = atoi(argv[4]), edge = atoi(argv[5]);
    const int n_bands = atoi(argv[6]), n_members = atoi(argv[7]);
    if (n_members < 1 || n_members > 16 || argc < 9 + n_members || frames < 100 || frames > 4096) {
        fprintf(stderr, "bad arguments\n");
        return 2;
    }
    int32_t devices[16];
    for (int m = 0; m < n_members; m++)
        devices[m] = (int32_t)atoi(argv[8 + m]);
    int a = 8 + n_members;
    if (strcmp(argv[a], "--") != 0) {
        fprintf(stderr, "expected -- before the bins\n");
        return 2;
    }
    int bins[MAX_BINS], n_bins = 0;
    for (a++; a < argc && n_bins < MAX_BINS; a++)
        bins[n_bins++] = atoi(argv[a]);
    const size_t n_floats = (size_t)n_bands * (size_t)frames * (size_t)n * 2u;
    float *iq = (float *)malloc(n_floats * sizeof(float));
    FILE *f = fopen(argv[1], "rb");
    if (!iq || !f || fread(iq, sizeof(float), n_floats, f) != n_floats) {
        fprintf(stderr, "cannot read %zu floats from %s\n", n_floats, argv[1]);
        return 2;
    }
    fclose(f);
    sdr_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.struct_size = (int32_t)sizeof cfg;
    cfg.n_bands = n_bands;
    cfg.sample_rate = rate;
    cfg.block_size = n;
    cfg.edge_width = edge;
    cfg.peak_threshold = SDR_DEFAULT_PEAK_THRESHOLD;
    cfg.signal_debounce = 1;
    cfg.max_listeners = MAX_BINS;
    cfg.max_batch_frames = frames;
    cfg.max_peaks = 64;
    cfg.find_peaks = 1;
    cfg.device_id = 99; /* ignored by a group: the members' devices are given */
    sdr_group *group = NULL;
    if (sdr_group_create(&cfg, devices, n_bands + 1, &group) != SDR_ERR_BAD_ARG) { /* more members than bands */
        fprintf(stderr, "n_bands < n_members not refused\n");
        return 1;
    }
    CHECK(sdr_group_create(&cfg, devices, n_members, &group));
    CHECK(sdr_group_enable_results(group, 1));
    int done = 0;
    CHECK(push_all(group, iq, n_bands, rate, n, frames, 0, 100));
    CHECK(sdr_group_process_staged(group, &done));
    if (done != 100) {
        fprintf(stderr, "processed %d of 100 frames\n", done);
        return 1;
    }
    if (deliver(group))
        return 1;
    for (int b = 0; b < n_bands; b++) {
        sdr_bank *bank = NULL;
        int local = -1;
        CHECK(sdr_group_member(group, b, &bank, &local));
        for (int i = 0; i < n_bins; i++) {
            int id = -1;
            CHECK(sdr_attach(bank, local, bins[i], &id));
            printf("attached band %d bin %d -> member %d local %d id %d\n", b, bins[i], b % n_members, local, id);
        }
    }
    CHECK(push_all(group, iq, n_bands, rate, n, frames, 100, frames - 100));
    CHECK(sdr_group_process_staged(group, &done));
    if (done != frames - 100) {
        fprintf(stderr, "processed %d of %d frames\n", done, frames - 100);
        return 1;
    }
    if (deliver(group))
        return 1;
    uint64_t runes_dropped = 1, edges_dropped = 1;
    CHECK(sdr_group_read_drop_counters(group, &runes_dropped, &edges_dropped));
    printf("total dropped %llu %llu\n", (unsigned long long)runes_dropped, (unsigned long long)edges_dropped);
    CHECK(sdr_group_destroy(group));
    free(iq);
    printf("done\n");
    return 0;
}
