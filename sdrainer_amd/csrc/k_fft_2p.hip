// k_fft_2p.hip — IQ frame -> float64 radix-2 DIT FFT -> fftshift -> PSD (float32) and the listener tap for N = 32768 and
// 65536, whose float64 frame (512 KB / 1 MB) fits neither the registers (512 KB) nor the LDS (160 KB) of one CU: two
// kernels over the two phases of fft_2p.h, the intermediate in a scratch buffer of the batch's set.
//
// A batch is run in frame groups: phase A of a group, then phase B of the same group, in stream order on the FFT stream
// (no workgroup waits for another).  The scratch holds one group's intermediate (16 bytes per sample); the group's size is
// the plan's (host/batch_plan.h fft2p_group_frames).
// Compiled with -ffp-contract=off (gomath.h).
#include <hip/hip_runtime.h>

#include "../../include/sdrainer_hip.h"
#include "fft_2p.h"
#include "fft_input.h"

// 8-bit input (iq8.h).  k_fft_2p_iq8.hip compiles this file again with SDR_FFT2P_IQ8 = 1: that unit holds phase A's
// 8-bit instances (k_fft2p_a / k_fft2p_win_a<LOGN, CS8 / CU8>) and launch_fft_2p_iq8, which runs them in front of THIS
// unit's phase B (launch_fft2p_b); this unit's kernels stay the four k_fft2p_a, the four k_fft2p_win_a and the two k_fft2p_b.
#if !defined(SDR_FFT2P_IQ8)
#define SDR_FFT2P_IQ8 0
#endif

namespace sdr {

__device__ __forceinline__ fft64::cplx tw_load(const fft64::cplx *__restrict__ tw, int i)
{
    return tw[i];
}

// Phase A (k_fft_2p_a.h): k_fft2p_a, and k_fft2p_win_a for a bank with a window
#define SDR_FFT2P_WIN 0
#include "k_fft_2p_a.h"
#undef SDR_FFT2P_WIN
#define SDR_FFT2P_WIN 1
#include "k_fft_2p_a.h"
#undef SDR_FFT2P_WIN

#if !SDR_FFT2P_IQ8
// Phase B of the same group: workgroup x = frame_local * WG_B + w takes the residues c = w G .. w G + G - 1, writes their
// bins' psd (fft-shifted) and the tap of the listeners whose bins are among them (k_fft_psd.hip "The tap"): the row's
// values of those residues go to LDS first, the tap reads them there.
template <int LOGN>
__global__ __launch_bounds__(fft2p::T) void k_fft2p_b(const fft64::cplx *__restrict__ y, const fft64::cplx *__restrict__ tw,
                                                      float *__restrict__ psd, int out_stride, int frame0, int group,
                                                      const int *__restrict__ tap_bins, float *__restrict__ tap_out, int n_tap, int tap_stride)
{
    using PH = fft2p::Phases<LOGN>;
    using S = typename PH::SB;
    constexpr int N = PH::N, MB = PH::B, A = PH::A;
    __shared__ double lr[S::G * S::LDS_ROW], li[S::G * S::LDS_ROW];
    const int fl = blockIdx.x / PH::WG_B, w = blockIdx.x % PH::WG_B, band = blockIdx.y, t = threadIdx.x;
    const int c0 = w * S::G;
    const auto W = [tw](int i) { return tw_load(tw, i); };
    double xr[fft2p::R], xi[fft2p::R];
    {
        const int gl = fft2p::p0_sub<MB>(t), c = c0 + gl;
        const fft64::cplx *__restrict__ in = y + ((size_t)band * group + fl) * N + c;
#pragma unroll
        for (int s = 0; s < fft2p::R; s++) {
            const fft64::cplx v = in[(size_t)fft2p::p0_index<MB>(t, s) << A];
            xr[s] = v.x;
            xi[s] = v.y;
        }
        fft2p::pass0<MB>(xr, xi, LOGN, A, c, t, W);
#pragma unroll
        for (int s = 0; s < fft2p::R; s++) {
            const int at = gl * S::LDS_ROW + fft2p::p0_index<MB>(t, s);
            lr[at] = xr[s];
            li[at] = xi[s];
        }
    }
    __syncthreads();
    const int gl = fft2p::p1_sub<MB, false>(t), c = c0 + gl;
#pragma unroll
    for (int s = 0; s < fft2p::R; s++) {
        const int at = gl * S::LDS_ROW + fft2p::p1_index<MB, false>(t, s);
        xr[s] = lr[at];
        xi[s] = li[at];
    }
    fft2p::pass1<MB, false>(xr, xi, LOGN, A, c, t, W);
    const int frame = frame0 + fl;
    float *__restrict__ row = psd + ((size_t)band * out_stride + frame) * N;
    float p[fft2p::R];
#pragma unroll
    for (int s = 0; s < fft2p::R; s++) {
        p[s] = fft2p::psd_of(xr[s], xi[s]);
        row[(c + (fft2p::p1_index<MB, false>(t, s) << A)) ^ (N / 2)] = p[s];
    }
    if (n_tap <= 0)
        return;  // (uniform)
    __syncthreads();  // every thread is done reading the exchange area
    float *prow = reinterpret_cast<float *>(lr);  // [residue of the workgroup][q]
#pragma unroll
    for (int s = 0; s < fft2p::R; s++)
        prow[gl * (1 << MB) + fft2p::p1_index<MB, false>(t, s)] = p[s];
    __syncthreads();
    const int *__restrict__ bins = tap_bins + (size_t)band * tap_stride;
    float *__restrict__ out = tap_out + ((size_t)band * out_stride + frame) * tap_stride;
    for (int l = t; l < n_tap; l += fft2p::T) {
        const int bin = bins[l];
        if (bin < 0) {
            if (w == 0)
                out[l] = 0.0f;
            continue;
        }
        const int idx = bin ^ (N / 2), cl = (idx & ((1 << A) - 1)) - c0;
        if (cl >= 0 && cl < S::G)
            out[l] = prow[cl * (1 << MB) + (idx >> A)];
    }
}

// phase B of frames [f0, f0 + g) of a group, behind their phase A on the same stream
hipError_t launch_fft2p_b(const FftLaunch &l, int f0, int g, LaunchAt at)
{
    const int group = l.fft.group_frames;
    if (l.logn == 15)
        launch_kernel((k_fft2p_b<15>), dim3(g * fft2p::Phases<15>::WG_B, l.n_bands), dim3(fft2p::T), 0, at, static_cast<const fft64::cplx *>(l.scratch), l.tw,
                      l.psd, l.out_stride, f0, group, l.tap.bins, l.tap.out, l.tap.n, l.tap.stride);
    else if (l.logn == 16)
        launch_kernel((k_fft2p_b<16>), dim3(g * fft2p::Phases<16>::WG_B, l.n_bands), dim3(fft2p::T), 0, at, static_cast<const fft64::cplx *>(l.scratch), l.tw,
                      l.psd, l.out_stride, f0, group, l.tap.bins, l.tap.out, l.tap.n, l.tap.stride);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}
#endif  // !SDR_FFT2P_IQ8

// A batch, frame group by frame group: launch_a(f0, g) launches phase A of frames [f0, f0 + g) on at.stream, phase B
// (k_fft_2p.hip's, for both units) follows it.  at.done rides on the last frame group's phase B, the last launch, and on
// nothing else.
template <class A>
static hipError_t launch_fft2p_groups(const FftLaunch &l, LaunchAt at, A launch_a)
{
    if (!l.fft.two_phase || l.fft.windowed != (l.window != nullptr))
        return hipErrorInvalidValue;
    if (l.n_frames <= 0 || l.n_bands <= 0)
        return hipSuccess;
    if (!l.scratch || l.fft.group_frames <= 0)
        return hipErrorInvalidValue;
    const int group = l.fft.group_frames;
    for (int f0 = 0; f0 < l.n_frames; f0 += group) {
        const int g = l.n_frames - f0 < group ? l.n_frames - f0 : group;
        launch_a(f0, g);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess)
            e = launch_fft2p_b(l, f0, g, f0 + group >= l.n_frames ? at : LaunchAt(at.stream));
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

#if !SDR_FFT2P_IQ8
template <int LOGN>
static hipError_t launch_fft2p_t(const FftLaunch &l, LaunchAt at)
{
    using PH = fft2p::Phases<LOGN>;
    const int group = l.fft.group_frames;
    const bool sc16 = l.fft.fmt == InFormat::SC16;
    return launch_fft2p_groups(l, at, [&](int f0, int g) {
        if (l.window && sc16)
            hipLaunchKernelGGL((k_fft2p_win_a<LOGN, InFormat::SC16>), dim3(g * PH::WG_A, l.n_bands), dim3(fft2p::T), 0, at.stream, l.iq, l.cur, l.tw,
                               l.scratch, l.in_stride, l.frame_stride, f0, group, l.window);
        else if (l.window)
            hipLaunchKernelGGL((k_fft2p_win_a<LOGN, InFormat::F32>), dim3(g * PH::WG_A, l.n_bands), dim3(fft2p::T), 0, at.stream, l.iq, l.cur, l.tw,
                               l.scratch, l.in_stride, l.frame_stride, f0, group, l.window);
        else if (sc16)
            hipLaunchKernelGGL((k_fft2p_a<LOGN, InFormat::SC16>), dim3(g * PH::WG_A, l.n_bands), dim3(fft2p::T), 0, at.stream, l.iq, l.cur, l.tw,
                               l.scratch, l.in_stride, l.frame_stride, f0, group);
        else
            hipLaunchKernelGGL((k_fft2p_a<LOGN, InFormat::F32>), dim3(g * PH::WG_A, l.n_bands), dim3(fft2p::T), 0, at.stream, l.iq, l.cur, l.tw,
                               l.scratch, l.in_stride, l.frame_stride, f0, group);
    });
}

// float32 and sc16 frames
hipError_t launch_fft_2p(const FftLaunch &l, LaunchAt at)
{
    if (l.fft.fmt != InFormat::F32 && l.fft.fmt != InFormat::SC16)
        return hipErrorInvalidValue;  // (k_fft_2p_iq8.hip's)
    switch (l.logn) {
    case 15: return launch_fft2p_t<15>(l, at);
    case 16: return launch_fft2p_t<16>(l, at);
    default: return hipErrorInvalidValue;
    }
}

#else  // SDR_FFT2P_IQ8
template <int LOGN, InFormat FMT>
static hipError_t launch_fft2p_t(const FftLaunch &l, LaunchAt at)
{
    using PH = fft2p::Phases<LOGN>;
    const int group = l.fft.group_frames;
    return launch_fft2p_groups(l, at, [&](int f0, int g) {
        if (l.window)
            hipLaunchKernelGGL((k_fft2p_win_a<LOGN, FMT>), dim3(g * PH::WG_A, l.n_bands), dim3(fft2p::T), 0, at.stream, l.iq, l.cur, l.tw, l.scratch,
                               l.in_stride, l.frame_stride, f0, group, l.window);
        else
            hipLaunchKernelGGL((k_fft2p_a<LOGN, FMT>), dim3(g * PH::WG_A, l.n_bands), dim3(fft2p::T), 0, at.stream, l.iq, l.cur, l.tw, l.scratch, l.in_stride,
                               l.frame_stride, f0, group);
    });
}

// cs8 and cu8 frames
hipError_t launch_fft_2p_iq8(const FftLaunch &l, LaunchAt at)
{
    const bool cu8 = l.fft.fmt == InFormat::CU8;
    if (!is_iq8(l.fft.fmt))
        return hipErrorInvalidValue;
    switch (l.logn) {
    case 15: return cu8 ? launch_fft2p_t<15, InFormat::CU8>(l, at) : launch_fft2p_t<15, InFormat::CS8>(l, at);
    case 16: return cu8 ? launch_fft2p_t<16, InFormat::CU8>(l, at) : launch_fft2p_t<16, InFormat::CS8>(l, at);
    default: return hipErrorInvalidValue;
    }
}
#endif  // SDR_FFT2P_IQ8

}  // namespace sdr
