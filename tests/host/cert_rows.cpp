// certify() (sdrainer_amd/csrc/noise_cert.h, the code k_psd_scan runs) on psd rows from a file, with the window sums formed
// in the reference's order, for tests/test_fuzz_paths_coverage.py: the tied-window frames of tests/fuzz_paths_gen.py must
// be refused by the certificate itself (no SDR_NOISE_FORCE_EXACT), and the literal loops must pick window 0.
// argv: file of float32 rows, n, edge; stdout: one line per row, "ok why exact_window".  No GPU, no HIP.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sdrainer_amd/csrc/noise_cert.h"

int main(int argc, char **argv)
{
    if (argc != 4)
        return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f)
        return 2;
    const int n = std::atoi(argv[2]), edge = std::atoi(argv[3]);
    noise::Geom g{n, edge, (n - 2 * edge) / 10, 0, 1.0 / ((double)n * (double)n)};
    g.n_windows = (n - 2 * edge) % 10 == 0 ? 9 : 10;  // (dsp/fft.go:228: a window is evaluated when the next one starts)
    std::vector<float> row(n);
    while (std::fread(row.data(), sizeof(float), n, f) == (size_t)n) {
        auto x_at = [&](int i) { return (double)row[i]; };
        double s1[noise::kMaxWindows] = {}, s2[noise::kMaxWindows] = {};
        for (int w = 0; w < g.n_windows; w++) {
            s1[w] = noise::window_sum(g, x_at, w);
            for (int i = 0; i < g.window; i++)
                s2[w] += x_at(edge + w * g.window + i) * x_at(edge + w * g.window + i);
        }
        const noise::Result r = noise::certify(s1, s2, g, x_at);
        const noise::Result e = noise::exact_frame(g, x_at, s1);
        std::printf("%d %d %d\n", r.ok ? 1 : 0, r.why, e.window);
    }
    std::fclose(f);
    return 0;
}
