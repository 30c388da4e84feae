// host::widen_frame (sdrainer_amd/csrc/host/delivery.h): the 64-bit bank frame index of a 32-bit frame word (sdr_edge.frame,
// sdr_results.rune_frames: the index modulo 2^32) against the first_frame of the batch that delivered it.  It inverts the
// cast for every frame within 2^31 - 1 of first_frame, on either side, with first_frame just below and just above each
// multiple of 2^32 (and of 2^31), and a plain cast does not.  No GPU, no library.
#include <cstdint>
#include <cstdio>

#include "../../sdrainer_amd/csrc/host/delivery.h"

int main()
{
    long checked = 0, failures = 0, cast_wrong = 0;
    const int64_t two31 = (int64_t)1 << 31, two32 = (int64_t)1 << 32;
    const int64_t distances[] = {0, 1, 2, 47, 48, 95, 96, 100, 65535, 65536, two31 - 2, two31 - 1};
    for (int64_t k = 0; k <= 6; k++)
        for (int64_t base : {k * two32, k * two32 + two31})
            for (int64_t off : {(int64_t)-100, (int64_t)-96, (int64_t)-2, (int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)2, (int64_t)96, (int64_t)100}) {
                const int64_t first = base + off;
                if (first < 0)
                    continue;
                for (int64_t d : distances)
                    for (int sign : {-1, 1}) {
                        const int64_t frame = first + sign * d;
                        if (frame < 0)
                            continue;
                        const uint32_t word = (uint32_t)frame;  // what the device stores
                        const int64_t got = host::widen_frame(word, first);
                        checked++;
                        if (got != frame) {
                            if (failures++ < 8)
                                printf("first_frame %lld frame %lld (word %u): widened to %lld\n", (long long)first, (long long)frame, word, (long long)got);
                        }
                        if ((uint32_t)got != word)
                            failures++;  // (the helper inverts the cast)
                        cast_wrong += (int64_t)word != frame;
                    }
            }
    // the header's expression, literally
    const int64_t first = 5 * two32 - 80;
    const uint32_t f32 = (uint32_t)(first + 100);
    if (host::widen_frame(f32, first) != first + (int32_t)(f32 - (uint32_t)first) || host::widen_frame(f32, first) != 5 * two32 + 20)
        failures++;
    printf("%ld frames widened, %ld of them beyond a plain cast, failures %ld\n", checked, cast_wrong, failures);
    return failures || !cast_wrong ? 1 : 0;
}
