// Host-only test of the batch plan at the block sizes of the two-phase FFT (sdrainer_amd/csrc/host/batch_plan.h):
// N = 32768 and 65536 take k_fft_2p (never k_fft_r32, never the wide tap, 128 MiB frame groups) and the chains' noise floor
// with its variance on the vector ALU (never the matrix pipe unless asked for), and N = 16384 keeps every choice it had.  Built by tests/test_block_size_wide.py.  No GPU, no HIP.
#include <cstdio>
#include <initializer_list>

#include "../../sdrainer_amd/csrc/host/batch_plan.h"

namespace {

int g_failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            g_failures++;                                                        \
        }                                                                        \
    } while (0)

constexpr int C = SDR_CUMULATION_SIZE;

sdr::BatchPlan plan(int bands, int n, int frames, int max_frames, int slots = 256, const sdr::Switches &sw = sdr::Switches())
{
    return sdr::plan_batch(sw, sdr::BatchGeometry{bands, n, max_frames, max_frames / C + 2}, frames, 0, false, slots);
}

}  // namespace

int main()
{
    // N = 16384: the choices of the parent (k_fft_r32 from 1024 frames with the wide tap, the scan, no frame groups)
    {
        const sdr::BatchPlan p = plan(1, 16384, 2048, 2048);
        CHECK(p.fft.r32 && p.fft.wide_tap && !p.fft.two_phase && p.fft.group_frames == 0);
        CHECK(p.noise_scan);
        const sdr::BatchPlan q = plan(1, 16384, 512, 2048);
        CHECK(!q.fft.r32 && !q.fft.wide_tap && !q.fft.two_phase && q.fft.group_frames == 0 && q.noise_scan);
        const sdr::BatchPlan r = plan(1, 16384, 2048, 2048, 600);
        CHECK(!r.fft.r32 && !r.fft.wide_tap && !r.fft.two_phase);
        for (int n = 512; n <= 16384; n *= 2)
            CHECK(!plan(1, n, 4096, 4096).fft.two_phase && plan(1, n, 4096, 4096).fft.group_frames == 0 && sdr::noise_scan_at(sdr::Switches(), n));
    }
    // N = 32768 / 65536: the two-phase kernels, psd columns for the refinement, the chains
    for (int n : {32768, 65536}) {
        for (int frames : {1, 333, 2048, 4096}) {
            const sdr::BatchPlan p = plan(1, n, frames, 4096);
            CHECK(p.fft.two_phase && !p.fft.r32 && !p.fft.wide_tap);
            CHECK(!p.noise_scan && !p.bound_done && !p.var_mfma);
            CHECK(p.fft.group_frames == (128 << 20) / (n * 16));
        }
        CHECK(!sdr::may_use_matrix_pipe(sdr::Switches(), n));
        sdr::Switches sw;
        sw.noise_scan = false;  // SDR_NOISE_PATH=chains: still the vector ALU at these sizes
        CHECK(!plan(1, n, 100, 4096, 16, sw).var_mfma && !sdr::may_use_matrix_pipe(sw, n));
        sw.var_mfma = 1;  // SDR_VAR_MFMA=1: the matrix pipe, probed at creation
        CHECK(plan(1, n, 100, 4096, 16, sw).var_mfma && sdr::may_use_matrix_pipe(sw, n));
        sw = sdr::Switches();
        sw.fft_r32 = 1;  // (forced on: N = 16384 only)
        CHECK(!plan(1, n, 4096, 4096, 16, sw).fft.r32);
        sw = sdr::Switches();
        sw.fft2p_group_mb = 0;  // the whole batch in one group
        CHECK(plan(3, n, 100, 700, 16, sw).fft.group_frames == 700);
        sw.fft2p_group_mb = 1;  // fewer bytes than one frame of three bands: one frame per group
        CHECK(plan(3, n, 100, 700, 16, sw).fft.group_frames == 1);
        CHECK(sdr::fft2p_group_frames(sdr::Switches(), n, 3, 4096) == (128 << 20) / (3 * n * 16));
        CHECK(sdr::fft2p_group_frames(sdr::Switches(), n, 1, 10) == 10);  // (never more than a batch holds)
        // the bound still follows the batch's size; its unit counts come from k_cum_bound (no scan)
        CHECK(plan(1, n, 2048, 4096).bound && !plan(1, n, 2048, 4096).bound_done);
        CHECK(!plan(1, n, 1024, 4096).bound || n == 65536);
    }
    // N <= 16384: the matrix pipe as before (short chain batches), and only when the chains were asked for
    {
        sdr::Switches sw;
        CHECK(!sdr::may_use_matrix_pipe(sw, 16384));
        sw.noise_scan = false;
        CHECK(sdr::may_use_matrix_pipe(sw, 16384) && plan(1, 16384, 2048, 4096, 16, sw).var_mfma && !plan(1, 16384, 4096, 4096, 16, sw).var_mfma);
    }
    // the scratch of a set (capi_bank.hip alloc_set) is sized by the same function the plan uses
    CHECK(sdr::fft2p_group_frames(sdr::Switches(), 16384, 1, 4096) == 0);
    std::printf(g_failures ? "FAILED %d\n" : "plan ok\n", g_failures);
    return g_failures ? 1 : 0;
}
