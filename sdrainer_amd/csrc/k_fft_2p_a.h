// k_fft_2p_a.h — phase A of the two-phase FFT (k_fft_2p.hip) as one kernel template over block size, input format and
// window, and the launcher of a batch's frame groups.
// Phase A of frames [frame0, frame0 + group) of band blockIdx.y: workgroup x = frame_local * WG_A + w takes the sub-FFTs
// p = w G .. w G + G - 1 (blocks k = brev_B(p)).  Y: [band][group frames][N].
//
// WIN... is empty or the bank's window table (sdr_set_window).  With it the kernel multiplies sample i of the frame by
// win[i] - one correctly rounded float32 multiplication per component, of the converted value for the narrow formats -
// where the plain kernel widens it.  One input loop serves every format (fft_input.h).  k_fft_2p.hip instantiates the
// launcher for F32 and SC16, k_fft_2p_iq8.hip for CS8 and CU8 (iq8.h: two bytes per sample); phase B is k_fft_2p.hip's
// for all of them (launch_fft2p_b).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/sdrainer_hip.h"
#include "fft_2p.h"
#include "fft_input.h"

namespace sdr {

__device__ __forceinline__ fft64::cplx tw_load(const fft64::cplx *__restrict__ tw, int i)
{
    return tw[i];
}

// the window's value for sample i (called with the kernel's WIN... pack, which holds the table)
__device__ __forceinline__ float window_value(const float *__restrict__ win, int i)
{
    return win[i];
}

template <int LOGN, InFormat FMT, class... WIN>
__global__ __launch_bounds__(fft2p::T) void k_fft2p_a(const void *__restrict__ iq_arg, const BatchCursor *__restrict__ cur,
                                                      const fft64::cplx *__restrict__ tw, fft64::cplx *__restrict__ y, size_t in_stride,
                                                      int frame_stride, int frame0, int group, WIN... win)
{
    static_assert(sizeof...(WIN) <= 1, "the window table or nothing");
    using PH = fft2p::Phases<LOGN>;
    using S = typename PH::SA;
    constexpr int N = PH::N, MB = PH::A;
    __shared__ double lr[S::G * S::LDS_ROW], li[S::G * S::LDS_ROW];
    const int fl = blockIdx.x / PH::WG_A, w = blockIdx.x % PH::WG_A, band = blockIdx.y, t = threadIdx.x;
    const size_t frame_at = input_sample_offset(band * in_stride, (unsigned)(frame0 + fl), frame_stride);  // (samples)
    const auto W = [tw](int i) { return tw_load(tw, i); };
    double xr[fft2p::R], xi[fft2p::R];
    {
        const int gl = fft2p::p0_sub<MB>(t), p = w * S::G + gl;
        // the format's word per sample, converted (fft_input.h) where the float32 frames are widened
        using IN = decltype(input_of<FMT>());
        constexpr IN in = input_of<FMT>();
        const typename IN::word *__restrict__ iq = input_frames<IN>(iq_arg, cur) + frame_at;
#pragma unroll
        for (int s = 0; s < fft2p::R; s++) {
            const int i = fft2p::a_sample<LOGN>(p, fft2p::p0_index<MB>(t, s));
            const typename IN::word v = iq[i];
            if constexpr (sizeof...(WIN) == 1) {
                const float wv = window_value(win..., i);
                xr[s] = (double)__fmul_rn(in.re(v), wv);
                xi[s] = (double)__fmul_rn(in.im(v), wv);
            } else {
                xr[s] = (double)in.re(v);
                xi[s] = (double)in.im(v);
            }
        }
        fft2p::pass0<MB>(xr, xi, LOGN, 0, 0, t, W);
#pragma unroll
        for (int s = 0; s < fft2p::R; s++) {
            const int at = gl * S::LDS_ROW + fft2p::p0_index<MB>(t, s);
            lr[at] = xr[s];
            li[at] = xi[s];
        }
    }
    __syncthreads();
    const int gl = fft2p::p1_sub<MB, true>(t);
#pragma unroll
    for (int s = 0; s < fft2p::R; s++) {
        const int at = gl * S::LDS_ROW + fft2p::p1_index<MB, true>(t, s);
        xr[s] = lr[at];
        xi[s] = li[at];
    }
    fft2p::pass1<MB, true>(xr, xi, LOGN, 0, 0, t, W);
    const int k = fft2p::a_block<LOGN>(w * S::G + gl);
    fft64::cplx *__restrict__ out = y + ((size_t)band * group + fl) * N + ((size_t)k << PH::A);
#pragma unroll
    for (int s = 0; s < fft2p::R; s++)
        out[fft2p::p1_index<MB, true>(t, s)] = fft64::cplx{xr[s], xi[s]};
}

// A batch, frame group by frame group: launch_a(f0, g) launches phase A of frames [f0, f0 + g) on at.stream, phase B
// (k_fft_2p.hip's, for every format) follows it.  at.done rides on the last frame group's phase B, the last launch, and on
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

template <int LOGN, InFormat FMT>
static hipError_t launch_fft2p_t(const FftLaunch &l, LaunchAt at)
{
    using PH = fft2p::Phases<LOGN>;
    const int group = l.fft.group_frames;
    return launch_fft2p_groups(l, at, [&](int f0, int g) {
        if (l.window)
            hipLaunchKernelGGL((k_fft2p_a<LOGN, FMT, const float *__restrict__>), dim3(g * PH::WG_A, l.n_bands), dim3(fft2p::T), 0, at.stream, l.iq, l.cur, l.tw,
                               l.scratch, l.in_stride, l.frame_stride, f0, group, l.window);
        else
            hipLaunchKernelGGL((k_fft2p_a<LOGN, FMT>), dim3(g * PH::WG_A, l.n_bands), dim3(fft2p::T), 0, at.stream, l.iq, l.cur, l.tw, l.scratch, l.in_stride,
                               l.frame_stride, f0, group);
    });
}

// N = 32768 / 65536, frames of format FMT with a window or without; any other format refused
template <InFormat FMT>
hipError_t launch_fft_2p(const FftLaunch &l, LaunchAt at)
{
    if (l.fft.fmt != FMT)
        return hipErrorInvalidValue;
    switch (l.logn) {
    case 15: return launch_fft2p_t<15, FMT>(l, at);
    case 16: return launch_fft2p_t<16, FMT>(l, at);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace sdr
