// k_fft_2p_a.h — phase A of the two-phase FFT (k_fft_2p.hip), plain and windowed: no include guard, see below.
// Phase A of frames [frame0, frame0 + group) of band blockIdx.y: workgroup x = frame_local * WG_A + w takes the sub-FFTs
// p = w G .. w G + G - 1 (blocks k = brev_B(p)).  Y: [band][group frames][N].
//
// k_fft_2p.hip includes this file twice.  SDR_FFT2P_WIN = 0: k_fft2p_a, whose tokens are what they were before the window
// existed.  SDR_FFT2P_WIN = 1: k_fft2p_win_a, which multiplies sample i of the frame by win[i] (sdr_set_window) - one
// correctly rounded float32 multiplication per component, of the converted value for sc16 input - where the plain kernel
// widens it.  One input loop serves every format (fft_input.h).  FMT = CS8 / CU8 (iq8.h: two bytes per sample) is
// instantiated by k_fft_2p_iq8.hip only.
#if SDR_FFT2P_WIN
#define SDR_K_FFT2P_A k_fft2p_win_a
#define SDR_FFT2P_WIN_PARAM , const float *__restrict__ win
#else
#define SDR_K_FFT2P_A k_fft2p_a
#define SDR_FFT2P_WIN_PARAM
#endif
template <int LOGN, InFormat FMT>
__global__ __launch_bounds__(fft2p::T) void SDR_K_FFT2P_A(const void *__restrict__ iq_arg, const BatchCursor *__restrict__ cur,
                                                      const fft64::cplx *__restrict__ tw, fft64::cplx *__restrict__ y, size_t in_stride,
                                                      int frame_stride, int frame0, int group SDR_FFT2P_WIN_PARAM)
{
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
#if SDR_FFT2P_WIN
            const float wv = win[i];
            xr[s] = (double)__fmul_rn(in.re(v), wv);
            xi[s] = (double)__fmul_rn(in.im(v), wv);
#else
            xr[s] = (double)in.re(v);
            xi[s] = (double)in.im(v);
#endif
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
#undef SDR_K_FFT2P_A
#undef SDR_FFT2P_WIN_PARAM
