// host/nco_table.h — the float32 (COS, SIN) table of include/sdrainer_hip.h's sdr_ddc_nco_table, built on the host: what the
// down-converter mixes with (capi_ddc.hip) and what the channelizer's FFT takes its twiddles from (capi_chan.hip).  No HIP
// include.
#pragma once
#include <cmath>
#include <vector>

#include "../../../include/sdrainer_hip.h"

namespace sdr {

// COS over one period from the quarter wave q[0 .. L/4] = cos(2 pi i / L), evaluated in float64 and rounded once, with the
// two ends set exactly; every other entry is a copy of one of these or its negation (both zeros are +0).
inline void build_nco(float *cos_out, float *sin_out)
{
    constexpr int L = SDR_DDC_NCO_SIZE, Q = L / 4;
    std::vector<float> c((size_t)L);
    for (int i = 0; i <= Q; i++)
        c[(size_t)i] = (float)std::cos(3.14159265358979323846264338327950288 * (double)i / (double)(L / 2));
    c[0] = 1.0f;
    c[(size_t)Q] = 0.0f;
    for (int i = Q + 1; i <= L / 2; i++)
        c[(size_t)i] = -c[(size_t)(L / 2 - i)];
    for (int i = L / 2 + 1; i < L; i++)
        c[(size_t)i] = c[(size_t)(L - i)];
    for (int i = 0; i < L; i++) {
        if (cos_out)
            cos_out[i] = c[(size_t)i];
        if (sin_out)
            sin_out[i] = c[(size_t)((i - Q + L) % L)];
    }
}

}  // namespace sdr
