// The host mirror's stream clock with overlapped frames (sdrainer_amd/csrc/host/rx.h FrameTiming), without a GPU: one frame
// advances the clock by hop / sample_rate, so a silent listener with silence time-out T is detached at the frame whose
// clock first exceeds T - at hop = N / 4 that is four times the frame of the hop = N run (up to the one-frame rounding of
// T * sample_rate / hop), not the same frame.
//   usage: test_overlap_clock <sample_rate> <block_size> <silence seconds>   prints "<hop> <frame>" for hop = N, N/2, N/4, N/16
#include <cstdio>
#include <cstdlib>

#include "../../sdrainer_amd/csrc/host/rx.h"

// the frame at which the receiver's segment loop detaches a listener bound before frame 0 that never writes: the first
// frame at which its time-out has fired, found twice - by FrameTiming::earliestExpiry (what Receiver::segmentLimit cuts
// the segment at) and by walking the frames one by one with Listener::TimeoutExceeded on the stream clock
static long long detach_frame(int rate, int n, int hop, double silence)
{
    rx::ManualClock clock;  // (the receiver's stream clock is one of these, set to frameTime(f) frame by frame)
    rx::Listener l("a", &clock, nullptr);
    l.SetSilenceTimeout(silence);
    l.SetAttachmentTimeout(1e18);
    rx::Peak p{};
    p.signal_bin = n / 3;
    l.Attach(p, 0);
    const rx::FrameTiming t{rate, hop};
    const long long predicted = t.earliestExpiry(l, 0);
    long long f = 0;
    for (;; f++) {
        clock.Set(t.frameTime(f));
        if (l.TimeoutExceeded())
            break;
    }
    if (f != predicted) {
        fprintf(stderr, "hop %d: walked to frame %lld, earliestExpiry says %lld\n", hop, f, predicted);
        exit(1);
    }
    return f;
}

int main(int argc, char **argv)
{
    if (argc < 4)
        return 2;
    const int rate = atoi(argv[1]), n = atoi(argv[2]);
    const double silence = atof(argv[3]);
    for (int hop : {n, n / 2, n / 4, n / 16})
        printf("%d %lld\n", hop, detach_frame(rate, n, hop, silence));
    return 0;
}
