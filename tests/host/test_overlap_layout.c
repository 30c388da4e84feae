/* include/sdrainer_hip.h from plain C11 (-Wall -Werror -pedantic): where sdr_config.hop lies - the word that was `reserved`,
 * so sizeof(sdr_config) stays what it was - and that the entry points of overlapped frames are declared with the
 * signatures a C caller uses.  Prints "sdr_config.hop <offset>" and "sizeof sdr_config <size>". */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "../../include/sdrainer_hip.h"

int main(void)
{
    int (*hop_of)(sdr_bank *) = sdr_hop;
    int (*stream_f32)(sdr_bank *, const float *, int, size_t) = sdr_process_device_stream;
    int (*stream_sc16)(sdr_bank *, const int16_t *, int, size_t) = sdr_process_device_stream_sc16;
    sdr_config cfg;
    memset(&cfg, 0, sizeof cfg); /* what every caller written before the field existed does: hop = 0 = block_size */
    printf("sdr_config.hop %d\n", (int)offsetof(sdr_config, hop));
    printf("sizeof sdr_config %d\n", (int)sizeof(sdr_config));
    printf("zeroed hop %d\n", (int)cfg.hop);
    printf("abi %d\n", SDR_ABI_VERSION);
    return hop_of && stream_f32 && stream_sc16 ? 0 : 1;
}
