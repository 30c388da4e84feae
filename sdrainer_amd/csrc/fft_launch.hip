// fft_launch.hip — the one dispatch of an FFT launch, and the twiddle and window tables of every block size.  Host code
// only: the kernels live in the eleven units whose launcher instances launch_fft picks from (k_fft_psd*.hip, k_fft_r32*.hip,
// k_fft_2p*.hip).  Which kernel runs is the batch plan's decision (host/batch_plan.h fft_choice -> fft_kernel); nothing is
// decided here.
#include <hip/hip_runtime.h>

#include "fft_f64.h"
#include "fft_r32.h"
#include "k_fft_psd.h"  // (window_slot; its launcher's instances are declared extern there, so no kernel is compiled here)
#include "sdr_device.h"

namespace sdr {

// The bank's twiddle buffer for N = 16384 holds both kernels' tables, the 32-point kernel's behind the other.
int twiddle_count(int logn)
{
    switch (logn) {
    case 9: return fft64::Plan<9>::TW_TOTAL;
    case 10: return fft64::Plan<10>::TW_TOTAL;
    case 11: return fft64::Plan<11>::TW_TOTAL;
    case 12: return fft64::Plan<12>::TW_TOTAL;
    case 13: return fft64::Plan<13>::TW_TOTAL;
    case 14: return fft64::Plan<14>::TW_TOTAL + fft32::kTwTotal;
    case 15: return 1 << 14;  // k_fft_2p: go-dsp's table as it is, the N / 2 entries a radix-2 FFT reads
    case 16: return 1 << 15;
    default: return 0;
    }
}

void build_twiddles(int logn, const double *wre, const double *wim, fft64::cplx *out)
{
    switch (logn) {
    case 9: fft64::build_pass_twiddles<9>(wre, wim, out); break;
    case 10: fft64::build_pass_twiddles<10>(wre, wim, out); break;
    case 11: fft64::build_pass_twiddles<11>(wre, wim, out); break;
    case 12: fft64::build_pass_twiddles<12>(wre, wim, out); break;
    case 13: fft64::build_pass_twiddles<13>(wre, wim, out); break;
    case 14:
        fft64::build_pass_twiddles<14>(wre, wim, out);
        fft32::build_twiddles(wre, wim, out + fft64::Plan<14>::TW_TOTAL);
        break;
    case 15:
    case 16:
        for (int i = 0; i < 1 << (logn - 1); i++)
            out[i] = fft64::cplx{wre[i], wim[i]};
        break;
    default: break;
    }
}

// The device image of a window table w[N] (sample order): the order the windowed kernel of that size reads it in.  N = 512
// - 16384: k_fft_psd.h load_window, slot m of thread t at window_slot(t, m).  N = 32768 / 65536: k_fft2p_a reads it in
// sample order beside the samples themselves.
template <int LOGN>
static void window_layout_t(const float *w, float *out)
{
    using PL = fft64::Plan<LOGN>;
    for (int t = 0; t < PL::T; t++)
        for (int m = 0; m < PL::R; m++)
            out[window_slot<LOGN>(t, m)] = w[fft64::input_sample<LOGN>(t, m)];
}
void window_layout(int logn, const float *w, float *out)
{
    switch (logn) {
    case 9: window_layout_t<9>(w, out); break;
    case 10: window_layout_t<10>(w, out); break;
    case 11: window_layout_t<11>(w, out); break;
    case 12: window_layout_t<12>(w, out); break;
    case 13: window_layout_t<13>(w, out); break;
    case 14: window_layout_t<14>(w, out); break;
    default:
        for (int i = 0; i < 1 << logn; i++)
            out[i] = w[i];
        break;
    }
}

#if !defined(SDR_FFT_TABLES_ONLY)  // (tools/fft_bench.hip, tools/fft_r32_bench.hip: the tables above beside one or two units' entries)
hipError_t launch_fft(const FftLaunch &l, LaunchAt at)
{
    using K = FftKernel;
    FftLaunch r32 = l;  // the k_fft_r32 units read the second table of the N = 16384 buffer
    r32.tw = l.tw + fft64::Plan<14>::TW_TOTAL;
    switch (fft_kernel(l.fft)) {
    case K::PSD: case K::PSD_MULTI: return launch_fft_psd<InF32, false>(l, at);
    case K::PSD_SC16: return launch_fft_psd<InSc16, false>(l, at);
    case K::PSD_WIN: case K::PSD_WIN_MULTI: return launch_fft_psd<InF32, true>(l, at);
    case K::PSD_SC16_WIN: return launch_fft_psd<InSc16, true>(l, at);
    case K::PSD_IQ8: return launch_fft_psd<InIq8, false>(l, at);
    case K::PSD_IQ8_WIN: return launch_fft_psd<InIq8, true>(l, at);
    case K::R32: return launch_fft_r32<InF32, false>(r32, at);
    case K::R32_SC16: return launch_fft_r32<InSc16, false>(r32, at);
    case K::R32_IQ8: return launch_fft_r32<InIq8, false>(r32, at);
    case K::R32_HOP: return launch_fft_r32<InF32, true>(r32, at);
    case K::R32_HOP_SC16: return launch_fft_r32<InSc16, true>(r32, at);
    case K::R32_HOP_IQ8: return launch_fft_r32<InIq8, true>(r32, at);
    case K::A2P_F32: case K::A2P_WIN_F32: return launch_fft_2p<InFormat::F32>(l, at);
    case K::A2P_SC16: case K::A2P_WIN_SC16: return launch_fft_2p<InFormat::SC16>(l, at);
    case K::A2P_CS8: case K::A2P_WIN_CS8: return launch_fft_2p<InFormat::CS8>(l, at);
    case K::A2P_CU8: case K::A2P_WIN_CU8: return launch_fft_2p<InFormat::CU8>(l, at);
    case K::COUNT: break;
    }
    return hipErrorInvalidValue;
}
#endif

}  // namespace sdr
