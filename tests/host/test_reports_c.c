/* sdr_listener_report from PLAIN C: its size and the offset of every field, one "name offset" line each, then "sizeof N"
 * (tests/test_reports_host.py compares them with the ctypes / numpy mirror of sdrainer_amd/capi.py), and the report entry
 * points taken by address with their declared types.  Compiles as C11 under -Wall -Werror -pedantic; needs no library. */
#include <stddef.h>
#include <stdio.h>

#include "../../include/sdrainer_hip.h"

_Static_assert(sizeof(sdr_listener_report) == 64, "sdr_listener_report is 64 bytes");
_Static_assert(sizeof(sdr_results) == 128, "sdr_results stays 128 bytes");
_Static_assert(SDR_ABI_VERSION == 2, "the ABI version stays 2");

#define FIELD(f) printf(#f " %zu\n", offsetof(sdr_listener_report, f))

int main(int argc, char **argv)
{
    int (*enable)(sdr_bank *, int) = sdr_enable_reports;
    int (*enabled)(sdr_bank *) = sdr_reports_enabled;
    int (*poll)(sdr_bank *, sdr_listener_report *, int, int *, int64_t *, int) = sdr_poll_reports;
    int (*genable)(sdr_group *, int) = sdr_group_enable_reports;
    int (*gpoll)(sdr_group *, sdr_listener_report *, int, int *, int64_t *, int) = sdr_group_poll_reports;
    (void)argv;
    if (argc > 64) /* (never: keeps the addresses alive without calling anything) */
        printf("%p %p %p %p %p\n", (void *)(size_t)enable, (void *)(size_t)enabled, (void *)(size_t)poll, (void *)(size_t)genable, (void *)(size_t)gpoll);
    FIELD(band);
    FIELD(listener);
    FIELD(bin);
    FIELD(ticks);
    FIELD(ticks_on);
    FIELD(ticks_off);
    FIELD(on_max_q);
    FIELD(reserved);
    FIELD(on_sum_q);
    FIELD(off_sum_q);
    FIELD(floor_sum_q);
    FIELD(wpm);
    printf("sizeof %zu\n", sizeof(sdr_listener_report));
    return 0;
}
