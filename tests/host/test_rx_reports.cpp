// The host mirror's listener reports (sdrainer_amd/csrc/host/rx.h: Receiver::EnableReports / ListenerLevel) on the device:
// a decode-mode receiver listens to one keyed carrier over a whole stream, fed in ragged pieces of at most max_batch frames
// (what the staging queue holds) and processed in segments of at most as many; the listener's totals since its Attach - each polled segment's record added up - are printed
// as JSON (wpm as the bits of its double).  tests/test_host_mirror_reports.py holds them against numpy over the oracle's
// whole-stream trace.
//   test_rx_reports <iq.f32> <rate> <n> <frames> <vfo_offset> <max_batch>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../sdrainer_amd/csrc/host/rx.h"

namespace {
struct CountingReporter : rx::Reporter {
    std::vector<std::string> events;
    void ListenerActivated(const std::string &l, int64_t f) override { events.push_back("+" + l + "@" + std::to_string(f)); }
    void ListenerDeactivated(const std::string &l, int64_t f) override { events.push_back("-" + l + "@" + std::to_string(f)); }
};
}  // namespace

int main(int argc, char **argv)
{
    if (argc != 7) {
        fprintf(stderr, "usage: %s <iq.f32> <rate> <n> <frames> <vfo_offset> <max_batch>\n", argv[0]);
        return 2;
    }
    const int rate = atoi(argv[2]), n = atoi(argv[3]), frames = atoi(argv[4]), max_batch = atoi(argv[6]);
    const long long vfo_offset = atoll(argv[5]);
    FILE *f = fopen(argv[1], "rb");
    if (!f)
        return 2;
    std::vector<float> iq((size_t)frames * 2 * (size_t)n);
    if (fread(iq.data(), sizeof(float), iq.size(), f) != iq.size())
        return 2;
    fclose(f);
    CountingReporter rep;  // must outlive the receiver: Stop() reports the final deactivation
    rx::Receiver r("rx", rx::DecodeMode);
    r.AddReporter(&rep);
    r.SetCenterFrequency(7020000);
    r.SetEdgeWidth(70 * n / 512);
    sdr_listener_report none{};
    if (r.EnableReports() != SDR_OK || r.ListenerLevel("rx1", &none))  // (before Start: stored; no listener is attached yet)
        return 3;
    if (r.Start(rate, n, max_batch) != SDR_OK || !sdr_reports_enabled(r.Bank())) {
        fprintf(stderr, "Start failed: %s\n", sdr_last_error());
        return 3;
    }
    if (r.SetVFOOffset(vfo_offset) != SDR_OK)
        return 4;
    const auto l = r.Listeners().First();
    if (!l || !l->Attached())
        return 4;
    sdr_listener_report t{};
    if (!r.ListenerLevel(l->ID(), &t) || t.ticks != 0 || t.on_max_q != INT32_MIN)  // cleared at Attach
        return 5;
    const int pieces[] = {1, 37, 100, 163, 7, 250};
    int done = 0, k = 0;
    while (done < frames) {
        const int m = std::min(std::min(pieces[k++ % 6], max_batch), frames - done);  // (the staging queue holds max_batch frames)
        if (r.IQData(rate, iq.data() + (size_t)done * 2 * n, (size_t)m * 2 * n) != SDR_OK || r.Process() != SDR_OK) {
            fprintf(stderr, "Process failed: %s\n", sdr_last_error());
            return 6;
        }
        done += m;
    }
    if (!r.ListenerLevel(l->ID(), &t))
        return 7;
    uint64_t wpm_bits;
    memcpy(&wpm_bits, &t.wpm, sizeof wpm_bits);
    printf("{\"frames\": %lld, \"id\": \"%s\", \"events\": %zu, \"band\": %d, \"listener\": %d, \"bin\": %d, \"ticks\": %d, \"ticks_on\": %d, "
           "\"ticks_off\": %d, \"on_max_q\": %d, \"on_sum_q\": %" PRId64 ", \"off_sum_q\": %" PRId64 ", \"floor_sum_q\": %" PRId64
           ", \"wpm_bits\": %" PRIu64 "}\n",
           (long long)r.FramesProcessed(), l->ID().c_str(), rep.events.size(), t.band, t.listener, t.bin, t.ticks, t.ticks_on, t.ticks_off,
           t.on_max_q, t.on_sum_q, t.off_sum_q, t.floor_sum_q, wpm_bits);
    // a retune detaches the listener: its totals go with it, the fresh one starts from nothing
    if (r.SetVFOOffset(vfo_offset) != SDR_OK)
        return 8;
    const auto l2 = r.Listeners().First();
    if (!l2 || !r.ListenerLevel(l2->ID(), &t) || t.ticks != 0 || t.ticks_on != 0 || t.on_sum_q != 0)
        return 9;
    return 0;
}
