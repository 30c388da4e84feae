// k_fft_2p.hip — IQ frame -> float64 radix-2 DIT FFT -> fftshift -> PSD (float32) and the listener tap for N = 32768 and
// 65536, whose float64 frame (512 KB / 1 MB) fits neither the registers (512 KB) nor the LDS (160 KB) of one CU: two
// kernels over the two phases of fft_2p.h, the intermediate in a scratch buffer of the batch's set.
//
// A batch is run in frame groups: phase A of a group, then phase B of the same group, in stream order on the FFT stream
// (no workgroup waits for another).  The scratch holds one group's intermediate (16 bytes per sample); the group's size is
// the plan's (host/batch_plan.h fft2p_group_frames).
// This unit holds phase B for every input format and phase A (k_fft_2p_a.h) for float32 and sc16 frames, plain and
// windowed; k_fft_2p_iq8.hip holds phase A for 8-bit frames.
// Compiled with -ffp-contract=off (gomath.h).
#include "k_fft_2p_a.h"

namespace sdr {

// Phase B of the same group: workgroup x = frame_local * WG_B + w takes the residues c = w G .. w G + G - 1, writes their
// bins' psd (fft-shifted) and the tap of the listeners whose bins are among them (k_fft_psd.h "The tap"): the row's
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

template hipError_t launch_fft_2p<InFormat::F32>(const FftLaunch &, LaunchAt);
template hipError_t launch_fft_2p<InFormat::SC16>(const FftLaunch &, LaunchAt);

}  // namespace sdr
