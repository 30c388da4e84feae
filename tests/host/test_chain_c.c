/* A PLAIN C caller of the receive chain (include/sdrainer_hip.h "receive chain"): compiled with gcc -std=c11 -Wall -Werror
 * -pedantic by tests/test_chain_c.py.  It takes the ten sdr_chain_* entry points by address with their declared types (the test
 * checks that every such declaration of the header is taken here), prints the size and every field offset of
 * sdr_chain_config and sdr_chain_counts ("size NAME BYTES", "field STRUCT NAME OFFSET"), which the test compares with the
 * ctypes structures, sees null handles and bad configurations refused without a GPU, and prints what the two host-only
 * calls make of a few arguments ("granule DTOT NB VALUE", "min_ring BLOCK HOP PIECE DTOT VALUE").
 */
#include <stddef.h>
#include <stdio.h>

#include "../../include/sdrainer_hip.h"

/* every entry point, by its declared type: a declaration that changes breaks this build */
static int (*const chain_create)(const sdr_chain_config *, sdr_chain **) = sdr_chain_create;
static int (*const chain_destroy)(sdr_chain *) = sdr_chain_destroy;
static int (*const chain_set_stream)(sdr_chain *, void *) = sdr_chain_set_stream;
static int (*const chain_sync)(sdr_chain *) = sdr_chain_sync;
static int (*const chain_push_host)(sdr_chain *, const void *, size_t, int *) = sdr_chain_push_host;
static int (*const chain_push_device)(sdr_chain *, const void *, size_t, int *) = sdr_chain_push_device;
static int (*const chain_read_narrow)(sdr_chain *, int, int64_t, int, float *) = sdr_chain_read_narrow;
static int (*const chain_stats)(sdr_chain *, sdr_chain_counts *) = sdr_chain_stats;
static int64_t (*const chain_granule)(int, int) = sdr_chain_granule;
static int64_t (*const chain_min_ring)(int, int, int64_t, int) = sdr_chain_min_ring;

_Static_assert(sizeof(sdr_chain_config) == 16 + 5 * sizeof(void *), "four words and five handles, no padding");
_Static_assert(sizeof(sdr_chain_counts) == 96, "sdr_chain_counts is 96 bytes");
_Static_assert(sizeof(sdr_ddc_config) == 32 && sizeof(sdr_chan_config) == 32 && sizeof(sdr_nb_config) == 32 && sizeof(sdr_fine_config) == 32,
               "the other config structs stay 32 bytes");

#define FIELD(s, f) printf("field " #s " " #f " %d\n", (int)offsetof(s, f))

int main(void)
{
    if (sdr_abi_version() != 2 || SDR_ABI_VERSION != 2) {
        fprintf(stderr, "sdr_abi_version is not 2\n");
        return 1;
    }
    printf("size sdr_chain_config %d\n", (int)sizeof(sdr_chain_config));
    FIELD(sdr_chain_config, struct_size);
    FIELD(sdr_chain_config, max_in_samples);
    FIELD(sdr_chain_config, ring_samples);
    FIELD(sdr_chain_config, reserved);
    FIELD(sdr_chain_config, nb);
    FIELD(sdr_chain_config, ddc);
    FIELD(sdr_chain_config, chan);
    FIELD(sdr_chain_config, fine);
    FIELD(sdr_chain_config, bank);
    printf("size sdr_chain_counts %d\n", (int)sizeof(sdr_chain_counts));
    FIELD(sdr_chain_counts, accepted);
    FIELD(sdr_chain_counts, processed);
    FIELD(sdr_chain_counts, pending);
    FIELD(sdr_chain_counts, narrow);
    FIELD(sdr_chain_counts, frames);
    FIELD(sdr_chain_counts, batches);
    FIELD(sdr_chain_counts, carry_moves);
    FIELD(sdr_chain_counts, granule);
    FIELD(sdr_chain_counts, piece);
    FIELD(sdr_chain_counts, ring_samples);
    FIELD(sdr_chain_counts, resident_from);
    FIELD(sdr_chain_counts, reserved);
    /* null handles are refused without a GPU */
    char raw[32] = {0};
    float out[8];
    int nb = -3;
    sdr_chain_counts counts;
    if (chain_set_stream(NULL, NULL) != SDR_ERR_BAD_ARG || chain_sync(NULL) != SDR_ERR_BAD_ARG ||
        chain_push_host(NULL, raw, 16, &nb) != SDR_ERR_BAD_ARG || chain_push_device(NULL, raw, 16, &nb) != SDR_ERR_BAD_ARG ||
        chain_read_narrow(NULL, 0, 0, 4, out) != SDR_ERR_BAD_ARG || chain_stats(NULL, &counts) != SDR_ERR_BAD_ARG ||
        chain_destroy(NULL) != SDR_OK || nb != -3) {
        fprintf(stderr, "a null handle was accepted\n");
        return 1;
    }
    /* and so is a configuration without members, before any device is touched */
    sdr_chain_config cfg = {sizeof(sdr_chain_config), 4096, 0, 0, NULL, NULL, NULL, NULL, NULL};
    sdr_chain *c = NULL;
    sdr_chain_config small = cfg, word = cfg, none = cfg;
    small.struct_size -= 8;
    word.reserved = 1;
    none.max_in_samples = 0;
    if (chain_create(NULL, &c) != SDR_ERR_BAD_ARG || chain_create(&cfg, NULL) != SDR_ERR_BAD_ARG || chain_create(&cfg, &c) != SDR_ERR_BAD_ARG ||
        chain_create(&small, &c) != SDR_ERR_BAD_ARG || chain_create(&word, &c) != SDR_ERR_BAD_ARG || chain_create(&none, &c) != SDR_ERR_BAD_ARG || c) {
        fprintf(stderr, "sdr_chain_create took a null pointer or a configuration without members\n");
        return 1;
    }
    static const int gr[][2] = {{1, 1}, {32, 1}, {32, 96}, {3, 64}, {8192, 4096}, {65536, 96}, {5, 1}, {0, 1}, {4, 0}, {-2, 64}, {4, -64}};
    for (size_t i = 0; i < sizeof gr / sizeof gr[0]; i++)
        printf("granule %d %d %lld\n", gr[i][0], gr[i][1], (long long)chain_granule(gr[i][0], gr[i][1]));
    static const long long mr[][4] = {{512, 128, 4096, 32},  {512, 512, 64, 32},  {8192, 512, 49152, 8192}, {512, 128, 70, 5},
                                      {512, 128, 4097, 32},  {512, 1024, 4096, 32}, {0, 128, 4096, 32},     {512, 0, 4096, 32},
                                      {512, 128, 0, 32},     {512, 128, 4096, 0},   {-512, 128, 4096, 32},  {512, 128, -4096, 32}};
    for (size_t i = 0; i < sizeof mr / sizeof mr[0]; i++)
        printf("min_ring %lld %lld %lld %lld %lld\n", mr[i][0], mr[i][1], mr[i][2], mr[i][3],
               (long long)chain_min_ring((int)mr[i][0], (int)mr[i][1], (int64_t)mr[i][2], (int)mr[i][3]));
    printf("layout ok\n");
    return 0;
}
