// The batch plan (sdrainer_amd/csrc/host/batch_plan.h, the library's own code) of every batch of a list of streams, for
// tests/test_fuzz_paths_coverage.py: what tests/test_gpu_fuzz_paths.py's default seeds make the scheduler choose.
// stdin: one line per batch, "n n_bands max_batch_frames n_frames count0 capturing max_slots"; stdout: one line per
// batch, "r32 wide_tap two_phase group_frames scan_parts gather_on_peaks noise_scan bound".  With --kernel on the command
// line the FFT kernel's name (fft_kernel_name, for float32 input and dense frames) follows as a ninth column.  No GPU, no HIP.
#include <cstdio>
#include <cstring>

#include "../../sdrainer_amd/csrc/host/batch_plan.h"

int main(int argc, char **argv)
{
    const bool with_kernel = argc > 1 && std::strcmp(argv[1], "--kernel") == 0;
    const sdr::Switches sw;  // (no switch set: every choice follows the batch's geometry)
    int n, n_bands, max_frames, n_frames, count0, capturing, max_slots;
    while (std::scanf("%d %d %d %d %d %d %d", &n, &n_bands, &max_frames, &n_frames, &count0, &capturing, &max_slots) == 7) {
        const sdr::BatchGeometry g{n_bands, n, max_frames, max_frames / SDR_CUMULATION_SIZE + 2};
        const sdr::BatchPlan p = sdr::plan_batch(sw, g, n_frames, count0, capturing != 0, max_slots);
        std::printf("%d %d %d %d %d %d %d %d", p.fft.r32 ? 1 : 0, p.fft.wide_tap ? 1 : 0, p.fft.two_phase ? 1 : 0, p.fft.group_frames,
                    p.scan_parts, p.stream[sdr::K_LISTEN_GATHER] == sdr::S_PEAKS ? 1 : 0, p.noise_scan ? 1 : 0, p.bound ? 1 : 0);
        std::printf(with_kernel ? " %s\n" : "\n", sdr::fft_kernel_name(sdr::fft_kernel(p.fft)));
    }
    return 0;
}
