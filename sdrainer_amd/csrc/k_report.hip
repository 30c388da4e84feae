// k_report.hip — listener reports (sdr_enable_reports / sdr_poll_reports): per batch and listener, how strong the listened
// signal was while the key was down and while it was up, the band's noise floor under the key-down ticks, and the decoder's
// speed - as counts, fixed-point sums and a maximum (include/sdrainer_hip.h sdr_listener_report), so that the bits depend
// on no schedule and the reports of consecutive batches add up.  Compiled with -ffp-contract=off.
//
// Two kernels on the decode stage's stream:
//   k_report_marks   in FRONT of k_listen_decode, a thread per slot: where in this batch the listener starts and from where
//                    its bin was tapped, clamped to [0, n_frames].  The decoder moves both marks of every started listener
//                    to the end of the batch (k_listen.hip, "Frame numbers are 32 bits ..."), so a kernel behind it cannot
//                    read them from the slot.
//   k_listen_report  BEHIND k_listen_decode and in front of k_pack_listen: the value of every tick exactly as
//                    k_listen_gather formed it (the same tap or retained psd value through the same gomath.h shortcut and
//                    literal fallback: its bit for bit), the debounced bit words the decoder left, the frame records' noise
//                    floor; the records go straight into the batch's block of pinned host memory.
#include <hip/hip_runtime.h>

#include <climits>

#include "../../include/sdrainer_hip.h"
#include "cw_decoder.h"
#include "gomath.h"
#include "sdr_device.h"

namespace sdr {

static_assert(sizeof(sdr_listener_report) == 64, "sdr_listener_report is 64 bytes (ABI)");

__global__ __launch_bounds__(256) void k_report_marks(const ListenerSlot *__restrict__ slots, const BatchCursor *__restrict__ cur,
                                                      uint32_t frame_base, int n_frames, int n_total, int32_t *__restrict__ marks)
{
    if (cur)  // graph replay: this batch's first frame comes from device memory
        frame_base = cur->frame_base;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_total)
        return;
    int skip = 0, untapped = 0;
    if (slots[idx].active) {
        // (frame numbers are 32 bits and compared as differences, as k_listen_gather compares them)
        skip = min(max((int)(slots[idx].start_frame - frame_base), 0), n_frames);
        untapped = min(max((int)(slots[idx].tapped_from - frame_base), 0), n_frames);
    }
    marks[2 * idx] = skip;
    marks[2 * idx + 1] = untapped;
}

// the literal Go algorithm, out of line (rare: about three values in 10^5 fail the shortcut's certificate)
__device__ __attribute__((noinline)) float report_db_slow(float psd, double inv_n2) { return gomath::psd_value_in_db(psd, inv_n2); }

// q(x) = (int32) rint(clamp(x, -1024, 1024) * 256): float32, round half to even, the product exact; x is not NaN
__device__ __forceinline__ int report_q(float x) { return (int)__builtin_rintf(fminf(fmaxf(x, -1024.f), 1024.f) * 256.f); }

// One workgroup per (band, 64 listener slots): lanes are slots - a wave reads 256 contiguous bytes of a tap row per
// instruction - and wave w walks the 64-frame words w, w + REPORT_WAVES, ...  Every lane keeps its partial integers in
// registers; the waves' partials meet in LDS and wave 0 adds them up and stores the 64-byte records.  No workgroup depends
// on another and nothing is accumulated in global memory: integer sums and maxima in any order are the same bits.
#ifndef SDR_REPORT_WAVES
#define SDR_REPORT_WAVES 8
#endif
constexpr int REPORT_WAVES = SDR_REPORT_WAVES;

__global__ __launch_bounds__(64 * REPORT_WAVES) void k_listen_report(const float *__restrict__ tap, const float *__restrict__ psd,
                                                                     const sdr_frame_rec *__restrict__ recs,
                                                                     const ListenerSlot *__restrict__ slots, const void *__restrict__ db_tab,
                                                                     const uint64_t *__restrict__ deb_bits, const int32_t *__restrict__ marks,
                                                                     ListenGeom g, int n_frames, int n_slots, double inv_n2,
                                                                     sdr_listener_report *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) unsigned char s_tab[gomath::kDbTabBytes];
    __shared__ long long s_on[REPORT_WAVES][64], s_off[REPORT_WAVES][64], s_floor[REPORT_WAVES][64];
    __shared__ int s_n_on[REPORT_WAVES][64], s_n_off[REPORT_WAVES][64], s_max[REPORT_WAVES][64];
    {
        const uint4 *src = static_cast<const uint4 *>(db_tab);
        uint4 *dst = reinterpret_cast<uint4 *>(s_tab);
        for (int i = threadIdx.x; i < gomath::kDbTabBytes / 16; i += blockDim.x)
            dst[i] = src[i];
    }
    __syncthreads();
    const gomath::DbTables tab = gomath::db_tables(s_tab);
    const int lane = threadIdx.x & 63, wave = (int)(threadIdx.x >> 6), band = blockIdx.y;
    const int l = blockIdx.x * 64 + lane;
    const size_t lidx = (size_t)band * g.max_listeners + (size_t)min(l, g.max_listeners - 1);
    const bool active = l < n_slots && slots[lidx].active != 0;
    const int skip = active ? marks[2 * lidx] : n_frames, untapped = active ? marks[2 * lidx + 1] : 0;
    const int bin = active ? slots[lidx].bin : 0;
    const size_t frame0 = (size_t)band * g.stride;
    const int n_words = (n_frames + 63) >> 6;
    long long on_sum = 0, off_sum = 0, floor_sum = 0;
    int n_on = 0, n_off = 0, on_max = INT_MIN;
    for (int word = wave; word < n_words; word += REPORT_WAVES) {
        const int f0 = word * 64, cnt = min(64, n_frames - f0);
        if (!active || f0 + cnt <= skip)  // (nothing of this word reaches the listener)
            continue;
        const uint64_t d = deb_bits[lidx * g.bit_words + word];
        for (int j0 = 0; j0 < cnt; j0 += 8) {
            float p[8], nf[8];
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int f = f0 + min(j0 + k, cnt - 1);
                p[k] = f < untapped ? psd[(frame0 + f) * (size_t)g.n + bin] : tap[(frame0 + f) * g.max_listeners + l];
                nf[k] = recs[frame0 + f].noise_floor;
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int j = j0 + k;
                if (j >= cnt || f0 + j < skip)
                    continue;
                float db;
                if (!gomath::psd_value_in_db_fast(p[k], tab, &db))
                    db = report_db_slow(p[k], inv_n2);
                const float v = db + (float)SDR_DBM_SHIFT;  // spectrum[SignalBin], the gather's value
                if (__builtin_isnan(v) || __builtin_isnan(nf[k]))
                    continue;  // an unmeasured tick
                const int q = report_q(v);
                if ((d >> j) & 1ull) {
                    n_on++;
                    on_sum += q;
                    floor_sum += report_q(nf[k]);
                    on_max = max(on_max, q);
                } else {
                    n_off++;
                    off_sum += q;
                }
            }
        }
    }
    s_on[wave][lane] = on_sum;
    s_off[wave][lane] = off_sum;
    s_floor[wave][lane] = floor_sum;
    s_n_on[wave][lane] = n_on;
    s_n_off[wave][lane] = n_off;
    s_max[wave][lane] = on_max;
    __syncthreads();
    if (wave != 0 || l >= n_slots)
        return;
    for (int w = 1; w < REPORT_WAVES; w++) {
        on_sum += s_on[w][lane];
        off_sum += s_off[w][lane];
        floor_sum += s_floor[w][lane];
        n_on += s_n_on[w][lane];
        n_off += s_n_off[w][lane];
        on_max = max(on_max, s_max[w][lane]);
    }
    sdr_listener_report r;
    r.band = band;
    r.listener = active ? l : -1;  // (-1: no listener in this slot - the host leaves the record out)
    r.bin = bin;
    r.ticks = active ? n_frames - skip : 0;
    r.ticks_on = n_on;
    r.ticks_off = n_off;
    r.on_max_q = on_max;
    r.reserved = 0;
    r.on_sum_q = on_sum;
    r.off_sum_q = off_sum;
    r.floor_sum_q = floor_sum;
    r.wpm = active ? slots[lidx].dec.wpm : 0.0;  // (the decoder of this batch has finished: same stream)
    out[(size_t)band * g.max_listeners + l] = r;
}

hipError_t launch_report_marks(const ListenerSlot *slots, const BatchCursor *cur, ListenGeom g, int n_frames, int n_bands, int32_t *marks,
                               hipStream_t stream)
{
    const int n_total = n_bands * g.max_listeners;
    if (n_total <= 0)
        return hipSuccess;
    hipLaunchKernelGGL(k_report_marks, dim3((n_total + 255) / 256), dim3(256), 0, stream, slots, cur, g.frame_base, n_frames, n_total, marks);
    return hipGetLastError();
}

hipError_t launch_listen_report(const float *tap, const float *psd, const sdr_frame_rec *recs, const ListenerSlot *slots, const void *db_tab,
                                const uint64_t *deb_bits, const int32_t *marks, ListenGeom g, int n_frames, int n_slots, int n_bands,
                                sdr_listener_report *out, hipStream_t stream)
{
    if (n_slots <= 0 || n_frames <= 0)
        return hipSuccess;
    if (n_slots > g.max_listeners || n_frames > g.stride || (n_frames + 63) / 64 > g.bit_words)
        return hipErrorInvalidValue;
    const double inv_n2 = 1.0 / ((double)g.n * (double)g.n);
    hipLaunchKernelGGL(k_listen_report, dim3((n_slots + 63) / 64, n_bands), dim3(64 * REPORT_WAVES), 0, stream, tap, psd, recs, slots, db_tab,
                       deb_bits, marks, g, n_frames, n_slots, inv_n2, out);
    return hipGetLastError();
}

}  // namespace sdr
