// The integer rule of sdr_fine_tune (sdrainer_amd/csrc/host/fine_tune.h) walked on the host, without the library and without
// a GPU: tests/test_fine_tune_host.py builds this plain and under the address and undefined-behaviour sanitizers.  Over every
// legal channelizer geometry and a dense set of targets (every target for the small ones) the result is compared with a
// search: the channel whose centre is nearest, the even one on a tie, the step as the remainder, 32768 wrapped to the next
// channel.  Illegal geometries and targets outside the wide stream are refused with the outputs untouched, at the ends of
// int64_t too.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../sdrainer_amd/csrc/host/fine_tune.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);       \
            failures++;                                                    \
        }                                                                  \
    } while (0)

static void by_search(int m, int d, int64_t target, int32_t *channel, int32_t *step)
{
    const int64_t q = 65536LL * d / m;
    int64_t best_c = 0, best = INT64_MAX;
    for (int64_t c = -m / 2 - 1; c <= m / 2 + 1; c++) {
        const int64_t dist = std::llabs(target - c * q);
        if (dist < best || (dist == best && (c & 1) == 0)) {
            best = dist;
            best_c = c;
        }
    }
    int64_t s = target - best_c * q;
    if (s == 32768) {
        best_c++;
        s = -32768;
    }
    *channel = (int32_t)(((best_c % m) + m) % m);
    *step = (int32_t)s;
}

int main()
{
    long long walked = 0;
    for (int m = 2; m <= 256; m *= 2)
        for (int d : {m, m / 2, m / 4}) {
            if (d < 1)
                continue;
            CHECK(sdr::fine_tune_geometry(m, d));
            CHECK(65536LL * d % m == 0);
            const int64_t edge = 32768LL * d, q = 65536LL * d / m;
            const int64_t stride = edge > 200000 ? 997 : 1;  // every target of the small geometries, a coprime walk otherwise
            for (int64_t target = -edge; target <= edge; target += stride) {
                int32_t c = -1, s = 0, wc = -2, ws = 1;
                CHECK(sdr::fine_tune(m, d, target, &c, &s));
                by_search(m, d, target, &wc, &ws);
                if (c != wc || s != ws) {
                    printf("FAILED M %d D %d target %lld: (%d, %d), by search (%d, %d)\n", m, d, (long long)target, c, s, wc, ws);
                    failures++;
                }
                CHECK(c >= 0 && c < m && s >= -32768 && s <= 32767 && 2 * (int64_t)std::abs(s) <= q);
                CHECK((((int64_t)c * q + s - target) % (65536LL * d)) == 0);
                walked++;
            }
            // round the ties and the edges, whatever the stride
            for (int64_t k = -m; k <= m; k++)
                for (int64_t off = -1; off <= 1; off++) {
                    const int64_t target = k * q / 2 + off;
                    int32_t c = -1, s = 0, wc = -2, ws = 1;
                    if (target < -edge || target > edge) {
                        CHECK(!sdr::fine_tune(m, d, target, &c, &s) && c == -1 && s == 0);
                        continue;
                    }
                    CHECK(sdr::fine_tune(m, d, target, &c, &s));
                    by_search(m, d, target, &wc, &ws);
                    CHECK(c == wc && s == ws);
                }
        }
    // refusals leave the outputs alone
    int32_t c = 11, s = 12;
    const int bad[][2] = {{0, 0}, {1, 1}, {2, 0}, {3, 3}, {6, 3}, {8, 1}, {8, 3}, {8, 16}, {8, -4}, {-8, -4}, {512, 128}, {512, 512}};
    for (const auto &g : bad) {
        CHECK(!sdr::fine_tune_geometry(g[0], g[1]));
        CHECK(!sdr::fine_tune(g[0], g[1], 0, &c, &s) && c == 11 && s == 12);
    }
    for (int64_t target : {(int64_t)32768 * 4 + 1, -(int64_t)32768 * 4 - 1, INT64_MAX, INT64_MIN, INT64_MAX / 2 + 1, INT64_MIN / 2 - 1})
        CHECK(!sdr::fine_tune(8, 4, target, &c, &s) && c == 11 && s == 12);
    CHECK(sdr::fine_tune(8, 4, 37568, &c, &s) && c == 1 && s == 4800);
    CHECK(sdr::fine_tune(8, 4, -71936, &c, &s) && c == 6 && s == -6400);
    CHECK(walked > 300000);
    if (failures == 0)
        printf("tune ok\n");
    return failures != 0;
}
