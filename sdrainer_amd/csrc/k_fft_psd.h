// k_fft_psd.h — the dominant kernel: IQ frame -> float64 radix-2 DIT FFT -> fftshift -> PSD (float32), plus the
// "tap": the PSD values of the bins the band's listeners sit on, gathered into a compact [frame][listener] array.
// The dB projection of dsp/fft.go:79-81 is a pure function of the float32 PSD value, so it is evaluated where it
// is consumed (k_peaks.hip cumulation, k_listen.hip envelope), not here: this kernel stores 4 bytes per sample
// instead of 8 and carries no logarithm.  Compiled with -ffp-contract=off (see gomath.h).
//
// Two kernel templates and their launcher.  k_fft_psd<LOGN, MULTI, WIN...> reads float32 frames, one per workgroup or
// several (MULTI); k_fft_psd_narrow<IN, LOGN, WIN, MORE...> reads the narrow formats (fft_input.h: InSc16, InIq8), one
// frame per workgroup, through fft_psd_one_frame.  launch_fft_psd<IN, WIN> launches the kernels of one format, plain or
// windowed, for N = 512 - 16384; three units instantiate it, two instances each: k_fft_psd.hip (float32 and sc16),
// k_fft_psd_win.hip (the same with a window) and k_fft_psd_iq8.hip (8-bit frames, plain and windowed).
//
// A window on the frames.  The windowed instances take the bank's window table (N float32 in device memory, in the order
// load_window reads it) as one more kernel argument - the WIN... pack holds it or nothing - and multiply sample i of every
// frame by its value: one correctly rounded float32 multiplication per component, where the plain kernels widen the sample
// to float64.  Everything behind the multiplication is the plain kernels'.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <tuple>
#include <type_traits>

#include "../../include/sdrainer_hip.h"
#include "cw_decoder.h"
#include "fft_f64.h"
#include "fft_input.h"
#include "fft_r32.h"
#include "gomath.h"
#include "sdr_device.h"

#if !defined(SDR_FFT_PSD_AUX)
#define SDR_FFT_PSD_AUX 0  // cache policy bits of the psd stores (2 = nt)
#endif
#if !defined(SDR_FFT_DMA_AUX)
#define SDR_FFT_DMA_AUX 2  // cache policy bits of the input LDS-DMA: nt - a frame is read once, by one CU (0.198 vs 0.202 ms)
#endif

namespace sdr {

// Development aids (tools/fft_bench.hip; none of this is compiled into the library).
//  SDR_FFT_PHASES=<workgroup>: every wave of that one workgroup reads the shader clock (s_memtime) at each phase
//    boundary into SGPRs - no wait, no store until the wave's last instruction - and writes the stamps out at the end;
//    the other workgroups pay a scalar compare per stamp.  (Round 2 stamped through memory at every boundary, which
//    cost a third of the kernel's speed; this costs under 1 %.)
//  SDR_FFT_CLOCK: per-workgroup spans (first wave's start, last wave's end, where it ran) + the in-kernel clock.
//  SDR_ABLATE=n: timing-only builds with one ingredient removed (results are wrong by construction).
// The stamps and spans go to g_fft_phases, sdr::g_fft_clock and sdr::g_fft_wg, device globals that the unit defines in
// front of this header: the tool, or k_fft_psd.hip in the diagnostic library build (SDR_FFT_CLOCK_LIB), which clocks that
// unit's kernels and no other's.
#if defined(SDR_FFT_CLOCK_LIB) && !defined(SDR_FFT_CLOCK_LIB_UNIT)
#undef SDR_FFT_CLOCK
#endif
// "Everything but the n youngest vector memory operations has completed": relies on loads, stores and LDS-DMA retiring
// in issue order (MI355X_MICROARCH.md; multi-frame workgroups only).  -DSDR_SAFE_FENCES waits for all of them instead.
#if defined(SDR_SAFE_FENCES)
#define SDR_WAIT_ALL_BUT(n) asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#else
#define SDR_WAIT_ALL_BUT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
#endif
enum StampId { ST_START = 0, ST_LOADED = 1, ST_PASS0 = 2, ST_EX0 = 3, ST_PASS1 = 4, ST_EX1 = 5, ST_PASS2 = 6, ST_EX2 = 7,
               ST_PASS3 = 8, ST_STORED = 10, ST_END = 11, ST_LANDED = 12, ST_ALL_LANDED = 13 };
#if defined(SDR_FFT_PHASES)
constexpr int kStampCount = 16;
struct Stamps {
    unsigned long long v[kStampCount];
    bool on;
};
#define SDR_STAMP(st, k)                                \
    do {                                                \
        if ((st).on)                                    \
            (st).v[k] = __builtin_amdgcn_s_memtime();   \
    } while (0)
#else
struct Stamps {
};
#define SDR_STAMP(st, k) \
    do {                 \
    } while (0)
#endif

// ---------------------------------------------------------------------------------------------
// k_fft_psd  (dsp/fft.go:23-37 IQToSpectrumAndPSD, the psd half; :59-69 setSamplesFromIQ; :54-57 fftshift)
// ---------------------------------------------------------------------------------------------
// Buffer addressing: address = descriptor base + per-thread 32-bit byte offset (a VGPR) + a scalar byte
// offset.  Everything that is the same for all threads - which register slot, which twiddle row - goes into
// the scalar offset, so a load or store costs no vector ALU instruction for its address.  The float64 VALU
// is this kernel's busiest unit; flat 64-bit addressing spent about 150 vector instructions per thread on
// address arithmetic.
using rsrc_t = __amdgpu_buffer_rsrc_t;
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ rsrc_t make_rsrc(const void *base, unsigned bytes)
{
    // inputs are made provably wave-uniform first, otherwise the descriptor is rebuilt per lane (waterfall)
    const unsigned long long b = (unsigned long long)base;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void *)(((unsigned long long)hi << 32) | lo), 0,
                                             __builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}

// Orders one wave's LDS stores before its later LDS loads (and the reverse) without a workgroup
// barrier: a wave's DS instructions execute in issue order, so the fences only pin the compiler.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// is the frame's last exchange through LDS the barrier-fenced cross-wave one?
template <int LOGN>
constexpr bool last_lds_exchange_is_cross()
{
    int last = -1;
    for (int e = 0; e < fft64::Plan<LOGN>::NPASS - 1; e++)
        if (!fft64::make_swap_plan<LOGN>(e).ok)
            last = e;
    return last >= 0 && fft64::Plan<LOGN>::cross_wave(last);
}

// Twiddles of a pass's first stages are requested BEFORE the exchange in front of the pass (SDR_FFT_TWPRE rows of the
// pass's twiddle block: 1 = stage 0, 3 = stages 0-1, 7 = stages 0-2): behind an exchange every wave of the
// workgroup starts its pass at the same moment, and without this each of them sat out an L2 round trip there - the
// fences of the exchange keep the compiler from hoisting the loads itself.  During the exchange only the 64 data
// registers are live, so the rows cost no register the pass does not have anyway.
#if !defined(SDR_FFT_TWPRE)
#define SDR_FFT_TWPRE 1
#endif
template <int LOGN, int P>
constexpr int tw_pre_rows()
{
    using PL = fft64::Plan<LOGN>;
    // (a short last pass has several groups per thread with different twiddles each, and nothing but register swaps
    // or nothing at all in front of it: left to the compiler)
    if (P <= 0 || P >= PL::NPASS || PL::pass_log(P) != PL::LOGR)
        return 0;
    constexpr int rows = (1 << PL::LOGR) - 1;
    return SDR_FFT_TWPRE < rows ? SDR_FFT_TWPRE : rows;
}
constexpr int kTwPreMax = 15;

__device__ __forceinline__ fft64::cplx load_tw(rsrc_t tw, int lo, int c)
{
    const u32x4 w = __builtin_amdgcn_raw_buffer_load_b128(tw, (unsigned)lo * 16u, c * 16, 0);
    fft64::cplx r;
    r.x = __hiloint2double((int)w.y, (int)w.x);
    r.y = __hiloint2double((int)w.w, (int)w.z);
    return r;
}

template <int LOGN, int P>
__device__ __forceinline__ void prefetch_tw(fft64::cplx (&pre)[kTwPreMax], int t, rsrc_t tw)
{
    using PL = fft64::Plan<LOGN>;
    constexpr int NPRE = tw_pre_rows<LOGN, P>();
    if constexpr (NPRE > 0) {
        constexpr int S = 1 << (P * PL::LOGR);
        const int lo = fft64::tw_pos<LOGN, P>(t, 0);
#pragma unroll
        for (int r = 0; r < NPRE; r++)
            pre[r] = load_tw(tw, lo, PL::tw_offset(P) + r * S);
    }
}

// Passes P .. NPASS-1 of one frame with the exchanges between them, on the thread's registers xr / xi.  `pre`: the first
// twiddle rows of pass P, requested before the exchange in front of it (pass 0 has none: its twiddles are scalar loads).
template <int LOGN, int P>
__device__ __forceinline__ void run_passes(double (&xr)[fft64::Plan<LOGN>::R], double (&xi)[fft64::Plan<LOGN>::R],
                                           int t, rsrc_t tw, const fft64::cplx *__restrict__ tw_ptr, double *lds,
                                           const fft64::cplx (&pre)[kTwPreMax], Stamps &st)
{
    using PL = fft64::Plan<LOGN>;
#if !(defined(SDR_ABLATE) && (SDR_ABLATE == 5))
    fft64::butterfly_pass<LOGN, P>(xr, xi, t, [tw, tw_ptr, &pre](int c, int lo) {
        if constexpr (P == 0)
            return tw_ptr[c];  // pass 0: the same entry for every thread, a scalar load
        constexpr int S = 1 << (P * PL::LOGR);
        const int row = (c - PL::tw_offset(P)) / S;  // (a constant once the pass is unrolled)
        if (row < tw_pre_rows<LOGN, P>())
            return pre[row];
        return load_tw(tw, lo, c);
    });
#endif
    fft64::cplx pre_next[kTwPreMax];
    if constexpr (P < PL::NPASS - 1)
        prefetch_tw<LOGN, P + 1>(pre_next, t, tw);
    SDR_STAMP(st, 2 + 2 * P);
    if constexpr (P < PL::NPASS - 1) {
        if constexpr (fft64::make_swap_plan<LOGN>(P).ok) {
            // done in registers (fft_f64.h exchange_swap: v_permlane16/32_swap), no LDS memory
#if !(defined(SDR_ABLATE) && (SDR_ABLATE == 14))
            fft64::exchange_swap<LOGN, P>(xr);
            fft64::exchange_swap<LOGN, P>(xi);
#endif
        } else {
            // A wave-local exchange (fft_f64.h make_layout) only touches LDS words of the wave's own
            // elements: no workgroup barrier, the waves drift apart and one wave's exchange overlaps the
            // others' butterflies.  The single cross-wave exchange is fenced by barriers on both sides.
            constexpr bool CROSS = PL::cross_wave(P);
            // timing-only builds: 10 = cross-wave exchange without its LDS traffic, 11 = without its barriers,
            // 12 = without either, 13 = no wave-local LDS exchange
#if defined(SDR_ABLATE) && (SDR_ABLATE == 11 || SDR_ABLATE == 12)
            constexpr bool BARRIERS = false;
#else
            constexpr bool BARRIERS = CROSS;
#endif
#if defined(SDR_ABLATE) && (SDR_ABLATE == 10 || SDR_ABLATE == 12)
            constexpr bool TRAFFIC = !CROSS;
#elif defined(SDR_ABLATE) && (SDR_ABLATE == 13)
            constexpr bool TRAFFIC = CROSS;
#else
            constexpr bool TRAFFIC = true;
#endif
            auto sync = [] {
                if constexpr (BARRIERS)
                    __syncthreads();
                else
                    wave_sync();
            };
            auto wr = [&](double (&x)[PL::R], double *area) {
                if constexpr (TRAFFIC)
                    fft64::exchange_write<LOGN, P>(x, t, area);
            };
            auto rd = [&](double (&x)[PL::R], double *area) {
                if constexpr (TRAFFIC)
                    fft64::exchange_read<LOGN, P>(x, t, area);
            };
            if constexpr (BARRIERS)
                __syncthreads();  // every wave is done with the words of its previous wave-local exchange
#if defined(SDR_ABLATE) && (SDR_ABLATE == 2)
            if (t < 0)  // timing-only build: no exchanges
#endif
            if constexpr (PL::SPLIT) {
                wr(xr, lds);
                sync();
                rd(xr, lds);
                sync();
                wr(xi, lds);
                sync();
                rd(xi, lds);
            } else {
                wr(xr, lds);
                wr(xi, lds + fft64::kExchangeWords<LOGN>);
                sync();
                rd(xr, lds);
                rd(xi, lds + fft64::kExchangeWords<LOGN>);
            }
            // reads done before LDS is written again: by a later exchange (other waves' words if CROSS), the next
            // frame's staging or the tap's copy of the psd row
            sync();
        }
        SDR_STAMP(st, 3 + 2 * P);
        run_passes<LOGN, P + 1>(xr, xi, t, tw, tw_ptr, lds, pre_next, st);
    }
}

// The window values of thread t's register slots (slot m holds sample input_sample(t, m)).  In sample order a wave's
// lanes would read them 32 bytes and more apart - what the frame itself avoids by going through LDS; measured, sixteen
// such dword loads per thread made the kernel 13 % slower per launch.  So the bank keeps the table in THIS kernel's order
// (fft_launch.hip window_layout, applied once by sdr_set_window): [m / 4][t][m % 4], a thread's four values of a slot group in one
// 16-byte load, a wave instruction reading 1 KB contiguous - R / 4 loads per thread.  Called before the wait for the
// frame's LDS-DMA: the loads ride under it (the table is L2-resident like the twiddles).
template <int LOGN>
SDR_HD constexpr int window_slot(int t, int m)
{
    return ((m >> 2) * fft64::Plan<LOGN>::T + t) * 4 + (m & 3);
}
template <int LOGN>
__device__ __forceinline__ void load_window(float (&wv)[fft64::Plan<LOGN>::R], int t, const float *__restrict__ win)
{
    using PL = fft64::Plan<LOGN>;
    static_assert(PL::R % 4 == 0 && PL::R * PL::T == PL::N, "the table holds R values per thread, four per load");
    const rsrc_t wrs = make_rsrc(win, PL::N * 4u);
    const unsigned woff = (unsigned)window_slot<LOGN>(t, 0) * 4u;
#pragma unroll
    for (int j = 0; j < PL::R / 4; j++) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrs, woff, window_slot<LOGN>(0, 4 * j) * 4, 0);
        wv[4 * j + 0] = __uint_as_float(v.x);
        wv[4 * j + 1] = __uint_as_float(v.y);
        wv[4 * j + 2] = __uint_as_float(v.z);
        wv[4 * j + 3] = __uint_as_float(v.w);
    }
}

// Epilogue (dsp/fft.go:54-57 fftshift, :71-73 PSD[float32]): psd[k] = float32(re^2 + im^2), two multiplies and an
// add in float64, no FMA, rounded once.
// LDS_COPY: the row also goes to LDS (float32 at byte 4 k), where the one-frame workgroup's tap picks its bins up.
template <int LOGN, bool LDS_COPY>
__device__ __forceinline__ void store_psd(const double (&xr)[fft64::Plan<LOGN>::R], const double (&xi)[fft64::Plan<LOGN>::R],
                                          int t, float *__restrict__ pd, unsigned char *lds_row, bool lds_copy)
{
    using PL = fft64::Plan<LOGN>;
    const int tp = fft64::thread_part<LOGN, PL::NPASS - 1>(t);
    // fft-shift = flip the top index bit: in the slot part it is a compile-time constant, in the thread part
    // it is applied once; spectrum index k = tk | sk(s), and sk(s) goes into the scalar offset
    constexpr int SLOT_MASK = fft64::slot_part<LOGN, PL::NPASS - 1>(PL::R - 1);
    constexpr int H = PL::N / 2;
    const unsigned tk = (unsigned)(tp ^ (H & ~SLOT_MASK));
    const rsrc_t pdr = make_rsrc(pd, PL::N * 4u);
#pragma unroll
    for (int s = 0; s < PL::R; s++) {
        const int sk = fft64::slot_part<LOGN, PL::NPASS - 1>(s) ^ (H & SLOT_MASK);
        const float p = (float)(xr[s] * xr[s] + xi[s] * xi[s]);
#if defined(SDR_ABLATE) && (SDR_ABLATE == 6 || SDR_ABLATE == 7 || SDR_ABLATE == 16)
        if (p == 1234.5f)  // timing-only build: (almost) no stores
            pd[tk | sk] = p;
#else
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(p), pdr, tk * 4u, sk * 4, SDR_FFT_PSD_AUX);
#endif
        if constexpr (LDS_COPY)
            if (lds_copy)  // (uniform) per-thread address once, the slot part in the instruction's offset field
                *reinterpret_cast<float *>(lds_row + tk * 4u + (unsigned)(sk * 4)) = p;
    }
}

// Where the time of a frame goes (N = 16384, tools/fft_bench.hip with -DSDR_FFT_CLOCK and the -DSDR_ABLATE
// builds, MI355X at 2.3 GHz in-kernel): the phases of a frame run one after the other on its CU - all 16 waves
// wait for the input, then all compute, then all exchange, ... - and each phase is bound by a different unit, so
// their times ADD: nothing of another frame can run beside them, a frame's float64 state is half the CU's
// register file.  Hence:
//  * MULTI: a workgroup takes `fpw` consecutive frames and has the next frame's LDS-DMA in flight while it
//    finishes the current one (issued just before the epilogue).  The wait at the top of the next frame is a
//    COUNTED vmcnt: the DMA is older than the R psd stores that followed it, and vector-memory operations retire
//    in order, so "all but the R youngest" covers the DMA without draining the stores.
//  * no logarithm here (see the file header) - it was a fifth of the kernel.
// Tried and measured no better: starting the first generation of workgroups staggered over a frame time (the
// theory was that 256 CUs reading at the same moment and storing at the same moment make HBM bursts; spreading
// them changed nothing), a persistent variant prefetching into the registers the epilogue frees (5 % slower).
//
// The tap.  `tap_bins[band][tap_stride]` lists the spectrum bins the band's listeners sit on (-1: free slot);
// for each of them the frame's psd value goes to tap_out[band][frame][slot].  The value is re-read from the psd
// row the workgroup has stored (thread l takes slot l), once those stores have certainly reached L2.  A MULTI
// workgroup taps frame f-1 near the end of frame f: by then every wave has waited for twiddles it loaded during
// frame f - younger than its stores of frame f-1, and vector-memory operations retire in order - and has passed
// the barriers of the cross-wave exchange since, so all of frame f-1's stores are complete; the tap then costs
// two instructions per listener and no drain; its last frame is tapped after a final drain.  A one-frame workgroup
// (the default) would pay that drain - a microsecond of store latency with the whole CU held - on every frame, so
// its epilogue also writes the psd row into LDS (the exchange area is free by then; LDS stores cost no vector ALU
// time) and the tap reads its bins from there behind one barrier: no wait on memory at all.
constexpr int kMaxLdsTap = 4096;  // listeners per band the LDS tap holds bins for (16 KB); more fall back to the drain

// the tap of one finished frame: slot l <- the row's value at the slot's bin, thread l takes slot l
template <int T>
__device__ __forceinline__ void tap_row(const float *row, const int *bins, float *out, int n_tap)
{
    for (int l = threadIdx.x; l < n_tap; l += T) {
        const int bin = bins[l];
        out[l] = bin >= 0 ? row[bin] : 0.0f;
    }
}

// The one-frame workgroup of k_fft_psd<LOGN, false> for the narrow input formats (fft_input.h: IN = InSc16, InIq8), the
// body of k_fft_psd_narrow.  Its LDS-DMA moves sizeof(IN::word) bytes per
// sample - R / 4 or R / 8 rows of 1 KB per wave - into the format's staging image, pass 0 reads one word per register
// slot and converts where the float32 kernel widens; WIN: one correctly rounded float32 multiplication of the converted
// value per component (load_window).  From the first butterfly on everything is the float32 kernel's (run_passes,
// store_psd, the LDS tap), so the results are the float32 path's bits for the converted values.  Only this one form
// exists for these formats: the multi-frame workgroup and the timing-only builds stay float32-only (launch_fft_t).
template <class IN, int LOGN, bool WIN>
__device__ __forceinline__ void fft_psd_one_frame(const IN in, const void *__restrict__ iq_arg, const BatchCursor *__restrict__ cur,
                                                  const fft64::cplx *__restrict__ tw, float *__restrict__ psd, size_t in_stride,
                                                  int frame_stride, int out_stride, const int *__restrict__ tap_bins,
                                                  float *__restrict__ tap_out, int n_tap, int tap_stride, const float *__restrict__ win)
{
    using PL = fft64::Plan<LOGN>;
    using IM = typename IN::template Image<LOGN>;
    using word = typename IN::word;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *lds = reinterpret_cast<double *>(smem);
    Stamps st;
#if defined(SDR_FFT_PHASES)
    st.on = false;
#endif
    const int frame = blockIdx.x;
    const size_t in_band = blockIdx.y * in_stride, out_band = (size_t)blockIdx.y * out_stride;
    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    {
        // frame -> LDS: row r = wave * ROWS_PER_WAVE + j; lane p fetches granule IM::granule(p, r) of the row (the swizzle
        // lives in the source address, the DMA writes lane p's 16 bytes at row base + 16 p); the descriptor ends with the frame
        const int lane = t & 63;
        const rsrc_t xrs = make_rsrc(input_frames<IN>(iq_arg, cur) + input_sample_offset(in_band, frame, frame_stride), PL::N * (unsigned)sizeof(word));
#pragma unroll
        for (int j = 0; j < IM::ROWS_PER_WAVE; j++) {
            const int r = wave * IM::ROWS_PER_WAVE + j;
            const int g = IM::granule(lane, r);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void *)(smem + r * 1024), 16,
                                                     (unsigned)g * 16u, r * 1024, 0, SDR_FFT_DMA_AUX);
        }
    }
    // the listeners' bins into LDS (behind the exchange area) while the frame is on its way
    int *lds_bins = reinterpret_cast<int *>(smem + fft64::kLdsBytes<LOGN>);
    const bool lds_tap = n_tap > 0 && n_tap <= kMaxLdsTap;
    if (lds_tap)
        for (int l = threadIdx.x; l < n_tap; l += PL::T)
            lds_bins[l] = tap_bins[(size_t)blockIdx.y * tap_stride + l];
    float wv[WIN ? PL::R : 1];
    if constexpr (WIN)
        load_window<LOGN>(wv, t, win);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    double xr[PL::R], xi[PL::R];
    {
        // dsp/fft.go:59-69 setSamplesFromIQ: slot m <- sample input_sample(t, m), the image address linear over GF(2)
        const int thread_byte = IM::lds_byte(fft64::input_sample<LOGN>(t, 0));
#pragma unroll
        for (int m = 0; m < PL::R; m++) {
            const int slot_byte = IM::lds_byte(fft64::input_sample<LOGN>(0, m));
            const word w = *reinterpret_cast<const word *>(smem + (thread_byte ^ slot_byte));
            if constexpr (WIN) {
                xr[m] = (double)__fmul_rn(in.re(w), wv[m]);
                xi[m] = (double)__fmul_rn(in.im(w), wv[m]);
            } else {
                xr[m] = (double)in.re(w);
                xi[m] = (double)in.im(w);
            }
        }
    }
    __syncthreads();  // everyone has its samples: the exchange area may be written again
    const fft64::cplx no_pre[kTwPreMax] = {};
    run_passes<LOGN, 0>(xr, xi, t, make_rsrc(tw, (unsigned)(PL::TW_TOTAL * sizeof(fft64::cplx))), tw, lds, no_pre, st);
    if constexpr (!last_lds_exchange_is_cross<LOGN>())
        if (lds_tap)
            __syncthreads();  // a wave-local last exchange fences only its own wave; the row goes everywhere
    store_psd<LOGN, true>(xr, xi, t, psd + (out_band + frame) * PL::N, smem, lds_tap);
    float *out = tap_out + (out_band + frame) * (size_t)tap_stride;
    if (lds_tap) {
        __syncthreads();  // the row is in LDS
        tap_row<PL::T>(reinterpret_cast<const float *>(smem), lds_bins, out, n_tap);
    } else if (n_tap > 0) {
        // more listeners than the LDS tap holds: re-read the stored row once it has reached memory
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        tap_row<PL::T>(psd + (out_band + frame) * PL::N, tap_bins + (size_t)blockIdx.y * tap_stride, out, n_tap);
    }
}

// the window table as a kernel argument: what the WIN... packs below hold, or nothing
using win_arg = const float *__restrict__;

// The float32 kernel.  WIN...: win_arg or nothing.
// (second launch bound = waves per SIMD the register allocation must leave room for: four, i.e. one 1024-thread
// workgroup or two 512-thread ones per CU)
template <int LOGN, bool MULTI, class... WIN>
__global__ __launch_bounds__(fft64::Plan<LOGN>::T, (fft64::Plan<LOGN>::T >= 512 ? 4 : 1)) void k_fft_psd(const float *__restrict__ iq_arg, const BatchCursor *__restrict__ cur,
                                                                  const fft64::cplx *__restrict__ tw,
                                                                  float *__restrict__ psd, size_t in_stride, int frame_stride, int out_stride,
                                                                  int n_frames, int fpw, const int *__restrict__ tap_bins,
                                                                  float *__restrict__ tap_out, int n_tap, int tap_stride, WIN... win)
{
#if defined(__HIP_DEVICE_COMPILE__)  // (the host pass needs the signature only; with the body it drops the stub without a diagnostic)
    static_assert(sizeof...(WIN) <= 1, "the window table or nothing");
    constexpr bool WINDOWED = sizeof...(WIN) == 1;
    using PL = fft64::Plan<LOGN>;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *lds = reinterpret_cast<double *>(smem);
    Stamps st;
#if defined(SDR_FFT_PHASES)
    st.on = blockIdx.x == SDR_FFT_PHASES && blockIdx.y == 0;
#pragma unroll
    for (int k = 0; k < kStampCount; k++)
        st.v[k] = 0;
#endif
#if defined(SDR_FFT_CLOCK)
    unsigned long long ck0 = 0, rt0 = 0;
    if (blockIdx.x == 100)
        ck0 = __builtin_amdgcn_s_memtime();
    rt0 = __builtin_amdgcn_s_memrealtime();
#endif
    SDR_STAMP(st, ST_START);
    const float *__restrict__ iq = cur ? cur->iq : iq_arg;  // graph replay: the batch's input pointer lives in device memory
    const int frame0 = MULTI ? blockIdx.x * fpw : blockIdx.x;
    const int frame_end = MULTI ? min(frame0 + fpw, n_frames) : frame0 + 1;
    const size_t in_band = blockIdx.y * in_stride, out_band = (size_t)blockIdx.y * out_stride;
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // Frame -> LDS by LDS-DMA: one contiguous 1 KB row per wave instruction, shaped through the source address
    // (fft_f64.h "Input staging"), the image lives in the exchange area.
    auto stage_frame = [&](int frame, int t) {
#if defined(SDR_ABLATE) && (SDR_ABLATE == 15 || SDR_ABLATE == 16)
        if (frame >= 0)  // timing-only build: no input DMA at all - what a perfectly hidden input would leave
            return;
#endif
        constexpr int ROWS_PER_WAVE = InF32::Image<LOGN>::ROWS_PER_WAVE;
        const int lane = t & 63;
#if defined(SDR_ABLATE) && (SDR_ABLATE == 8)
        const size_t fr = (size_t)((blockIdx.y * (in_stride / PL::N) + frame) & 15) * PL::N;  // timing-only: 16 frames, L2-resident
#else
        const size_t fr = input_sample_offset(in_band, frame, frame_stride);
#endif
        // buffer form: row in the scalar offset, granule in one 32-bit VGPR - no 64-bit per-lane addresses
        const rsrc_t xrs = make_rsrc(iq + fr * 2, PL::N * 8u);
#pragma unroll
        for (int j = 0; j < ROWS_PER_WAVE; j++) {
            const int r = wave * ROWS_PER_WAVE + j;
            const int g = InF32::Image<LOGN>::granule(lane, r);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(xrs, (__attribute__((address_space(3))) void *)(smem + r * 1024), 16,
                                                     (unsigned)g * 16u, r * 1024, 0, SDR_FFT_DMA_AUX);
        }
    };
    // tap of one finished frame (its psd stores are known to be complete, see above)
    auto tap_frame = [&](int frame) {
        tap_row<PL::T>(psd + (out_band + frame) * PL::N, tap_bins + (size_t)blockIdx.y * tap_stride,
                       tap_out + (out_band + frame) * (size_t)tap_stride, n_tap);
    };
    stage_frame(frame0, tid);
    // one-frame workgroup: its listeners' bins into LDS (behind the exchange area) while the frame is on its way
    int *lds_bins = reinterpret_cast<int *>(smem + fft64::kLdsBytes<LOGN>);
    const bool lds_tap = !MULTI && n_tap > 0 && n_tap <= kMaxLdsTap;
    if (lds_tap)
        for (int l = threadIdx.x; l < n_tap; l += PL::T)
            lds_bins[l] = tap_bins[(size_t)blockIdx.y * tap_stride + l];

#pragma nounroll
    for (int frame = frame0; frame < frame_end; frame++) {
        // (with more than one frame per workgroup everything derived from the thread id is loop-invariant and the
        // compiler would hoist - and spill - it: make the thread id opaque per frame)
        int t = tid;
        if constexpr (MULTI)
            asm volatile("" : "+v"(t));
        // The first frame's DMA is the wave's only traffic: full drain.  A later frame's DMA is older than the
        // previous frame's R psd stores (MI355X_MICROARCH.md: loads, stores and LDS-DMA count together, in issue
        // order), so "all but the R youngest" covers it (tap traffic behind the stores only makes the wait cover
        // some of the stores too).
        double xr[PL::R], xi[PL::R];
        // (a later frame of a multi-frame workgroup: these loads are the youngest, so the counted wait below covers the
        // previous frame's stores as well as the DMA)
        float wv[WINDOWED ? PL::R : 1];
        if constexpr (WINDOWED)
            load_window<LOGN>(wv, t, win...);
        if (!MULTI || frame == frame0)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else
            SDR_WAIT_ALL_BUT(PL::R);
        SDR_STAMP(st, ST_LANDED);  // this wave's rows have landed
        __syncthreads();
        SDR_STAMP(st, ST_ALL_LANDED);  // everybody's have

        const int thread_byte = InF32::Image<LOGN>::lds_byte(fft64::input_sample<LOGN>(t, 0));
#pragma unroll
        for (int m = 0; m < PL::R; m++) {
#if defined(SDR_ABLATE) && (SDR_ABLATE == 1 || SDR_ABLATE == 7)
            const float2 v = make_float2(1e-3f * (float)(t + m), 0.5f);  // timing-only build: no input
#else
            // sample number -> image address is linear over GF(2): thread part and slot part combine by XOR, and the
            // slot part is a compile-time constant
            const int slot_byte = InF32::Image<LOGN>::lds_byte(fft64::input_sample<LOGN>(0, m));
            const float2 v = *reinterpret_cast<const float2 *>(smem + (thread_byte ^ slot_byte));
#endif
            if constexpr (WINDOWED) {
                xr[m] = (double)__fmul_rn(v.x, wv[m]);
                xi[m] = (double)__fmul_rn(v.y, wv[m]);
            } else {
                xr[m] = (double)v.x;
                xi[m] = (double)v.y;
            }
        }
        __syncthreads();  // everyone has its samples: the exchange area may be written again
        SDR_STAMP(st, ST_LOADED);
        const bool more = MULTI && frame + 1 < frame_end;
        // (no scheduling pin around the DMA: the compiler keeps it behind the exchanges' LDS accesses and behind the
        // twiddle loads already issued, which it waits for with counted vmcnt; a "memory" pin cost 46 spills)
        // (LDS is written again after the last exchange in both variants - the next frame's staging or the tap's
        // copy of the psd row - so the exchange ends with its fence: a barrier when it crossed waves)
        const fft64::cplx no_pre[kTwPreMax] = {};
        run_passes<LOGN, 0>(xr, xi, t, make_rsrc(tw, (unsigned)(PL::TW_TOTAL * sizeof(fft64::cplx))), tw, lds, no_pre, st);
        if constexpr (MULTI)
            if (more)
                stage_frame(frame + 1, t);
        if constexpr (!MULTI && !last_lds_exchange_is_cross<LOGN>())
            if (lds_tap)
                __syncthreads();  // a wave-local last exchange fences only its own wave; the row goes everywhere
        store_psd<LOGN, !MULTI>(xr, xi, t, psd + (out_band + frame) * PL::N, smem, lds_tap);
        // (behind the DMA and the stores, so that its two dependent loads delay neither: the oldest waves - the
        // ones that tap - reach the end of a frame microseconds before the youngest)
        if constexpr (MULTI) {
            static_assert(PL::NPASS >= 2, "the tap relies on pass-1 twiddle loads");
            if (n_tap > 0 && frame > frame0)
                tap_frame(frame - 1);
        }
        SDR_STAMP(st, ST_STORED);
    }
    if (lds_tap) {
        __syncthreads();  // the row is in LDS (and lds_bins has been for a long time)
        // (not tap_row: through it the compiler orders two instructions of this loop differently at N >= 4096)
        const float *row = reinterpret_cast<const float *>(smem);
        float *out = tap_out + (out_band + frame0) * (size_t)tap_stride;
        for (int l = threadIdx.x; l < n_tap; l += PL::T) {
            const int bin = lds_bins[l];
            out[l] = bin >= 0 ? row[bin] : 0.0f;
        }
    } else if (n_tap > 0 && frame_end > frame0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        tap_frame(frame_end - 1);
    }
    SDR_STAMP(st, ST_END);
#if defined(SDR_FFT_PHASES)
    if (st.on && (threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < kStampCount; k++)
            g_fft_phases[threadIdx.x >> 6][k] = st.v[k];
    }
#endif
#if defined(SDR_FFT_CLOCK)
    if (blockIdx.x == 100 && threadIdx.x == 0) {
        g_fft_clock[0] = __builtin_amdgcn_s_memtime() - ck0;
        g_fft_clock[1] = __builtin_amdgcn_s_memrealtime() - rt0;
    }
    // every workgroup: first wave's start, each wave's end (the host takes the latest), where it ran
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 2048) {
        const unsigned long long now = __builtin_amdgcn_s_memrealtime();
        if (threadIdx.x == 0) {
            g_fft_wg[blockIdx.x][0] = rt0;
            g_fft_wg[blockIdx.x][1] = now;
            // HW_REG_HW_ID: cu_id bits 11:8, sh_id 12, se_id 15:13 (gfx9); XCC_ID is a register of its own
            g_fft_wg[blockIdx.x][3] = __builtin_amdgcn_s_getreg((4 /*HW_ID*/) | (0 << 6) | (31 << 11)) |
                                      ((unsigned long long)__builtin_amdgcn_s_getreg((20 /*XCC_ID*/) | (0 << 6) | (3 << 11)) << 32);
        }
        atomicMax(&g_fft_wg[blockIdx.x][2], now);
    }
#endif
#endif  // __HIP_DEVICE_COMPILE__
}

// What a narrow format's kernel takes behind the common arguments, and the trait and the window table they make.  sc16
// (sc16.h: int16 I, int16 Q per sample): the window table when windowed, nothing otherwise.  8-bit (iq8.h: one byte I, one
// byte Q per sample, cs8 or cu8): flip / c (iq8::Format) and the table, null without a window.
template <class IN>
struct NarrowInput {
    IN in;
    const float *__restrict__ win;
};
__device__ __forceinline__ NarrowInput<InSc16> narrow_input() { return {InSc16{}, nullptr}; }
__device__ __forceinline__ NarrowInput<InSc16> narrow_input(win_arg win) { return {InSc16{}, win}; }
__device__ __forceinline__ NarrowInput<InIq8> narrow_input(unsigned flip, float c, win_arg win) { return {InIq8{{flip, c}}, win}; }

// k_fft_psd for the narrow formats: fft_psd_one_frame over IN.  MORE...: narrow_input's arguments for IN and WIN.
template <class IN, int LOGN, bool WIN, class... MORE>
__global__ __launch_bounds__(fft64::Plan<LOGN>::T, (fft64::Plan<LOGN>::T >= 512 ? 4 : 1)) void k_fft_psd_narrow(const typename IN::word *__restrict__ iq_arg, const BatchCursor *__restrict__ cur,
                                                                       const fft64::cplx *__restrict__ tw, float *__restrict__ psd,
                                                                       size_t in_stride, int frame_stride, int out_stride, const int *__restrict__ tap_bins,
                                                                       float *__restrict__ tap_out, int n_tap, int tap_stride, MORE... more)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const NarrowInput<IN> a = narrow_input(more...);
    fft_psd_one_frame<IN, LOGN, WIN>(a.in, iq_arg, cur, tw, psd, in_stride, frame_stride, out_stride, tap_bins, tap_out, n_tap, tap_stride, a.win);
#endif  // __HIP_DEVICE_COMPILE__
}

static_assert(fft32::T == kR32MaxTap, "host/batch_plan.h: k_fft_r32 serves one listener slot per thread");

// The kernels of launch_fft_psd<IN, WIN> and the plan's names for them (host/batch_plan.h fft_kernel).  The arguments an
// instance's kernels take behind the common ones come as a tuple (more_args), the kernel templates' packs are its types.
namespace psd {

template <class IN, bool WIN>
auto more_args(const FftLaunch &l)
{
    if constexpr (std::is_same_v<IN, InIq8>) {
        const iq8::Format f = iq8::format_of(l.fft.fmt == InFormat::CU8);
        return std::tuple<unsigned, float, win_arg>(f.flip, f.c, l.window);  // (l.window is null for the plain instance)
    } else if constexpr (WIN) {
        return std::tuple<win_arg>(l.window);
    } else {
        return std::tuple<>();
    }
}
// (the narrow formats have the one-frame form only: MULTI names the same kernel and the same id)
template <class IN, int LOGN, bool WIN, bool MULTI, class... MORE>
constexpr auto kernel_taking(std::tuple<MORE...>)
{
    if constexpr (std::is_same_v<IN, InF32>)
        return &k_fft_psd<LOGN, MULTI, MORE...>;
    else
        return &k_fft_psd_narrow<IN, LOGN, WIN, MORE...>;
}
template <class IN, bool WIN, bool MULTI>
constexpr FftKernel kernel_id()
{
    if constexpr (std::is_same_v<IN, InIq8>)
        return WIN ? FftKernel::PSD_IQ8_WIN : FftKernel::PSD_IQ8;
    else if constexpr (std::is_same_v<IN, InSc16>)
        return WIN ? FftKernel::PSD_SC16_WIN : FftKernel::PSD_SC16;
    else if constexpr (MULTI)
        return WIN ? FftKernel::PSD_WIN_MULTI : FftKernel::PSD_MULTI;
    else
        return WIN ? FftKernel::PSD_WIN : FftKernel::PSD;
}

}  // namespace psd

// The kernels of <IN, WIN> at one size: float32 frames, one per workgroup or several; or the narrow format's one kernel.
// WIN: the windowed kernels and l.window, in window_layout's order.
template <class IN, bool WIN, int LOGN>
static hipError_t launch_fft_t(const FftLaunch &l, LaunchAt at)
{
    using PL = fft64::Plan<LOGN>;
    constexpr bool F32 = std::is_same_v<IN, InF32>;
    const FftTap &tap = l.tap;
    const FftKernel k = fft_kernel(l.fft);
    const bool mine = (k == psd::kernel_id<IN, WIN, false>() || k == psd::kernel_id<IN, WIN, true>()) && WIN == (l.window != nullptr);
    const auto more = psd::more_args<IN, WIN>(l);
    // every kernel this instance can launch (a narrow format: the one kernel under both names)
    const auto one = psd::kernel_taking<IN, LOGN, WIN, false>(more), multi = psd::kernel_taking<IN, LOGN, WIN, true>(more);
    static LdsLimitOnce lds_once;
    const hipError_t attr_err = raise_lds_limit_once(lds_once, {reinterpret_cast<const void *>(one), reinterpret_cast<const void *>(multi)},
                                                     fft64::kLdsBytes<LOGN> + kMaxLdsTap * 4);
    if (attr_err != hipSuccess)
        return attr_err;
    if (!mine)
        return hipErrorInvalidValue;
    if (l.n_frames <= 0 || l.n_bands <= 0)
        return hipSuccess;
    const unsigned tap_lds = tap.n > 0 && tap.n <= kMaxLdsTap ? ((tap.n * 4 + 255) & ~255) : 0;
    // (a kernel's arguments: the common ones, then the instance's own)
    const auto launch = [&](auto kernel, dim3 grid, unsigned lds_bytes, auto... common) {
        std::apply([&](auto... own) { launch_kernel(kernel, grid, dim3(PL::T), lds_bytes, at, common..., own...); }, more);
    };
    if constexpr (F32) {
        const float *iq = static_cast<const float *>(l.iq);
        const int fpw = l.fft.frames_per_wg;  // (host/batch_plan.h fft_frames_per_wg; a workgroup's frames are consecutive)
        if (k == psd::kernel_id<IN, WIN, true>())
            launch(multi, dim3((l.n_frames + fpw - 1) / fpw, l.n_bands), fft64::kLdsBytes<LOGN>, iq, l.cur, l.tw, l.psd, l.in_stride, l.frame_stride,
                   l.out_stride, l.n_frames, fpw, tap.bins, tap.out, tap.n, tap.stride);
        else
            launch(one, dim3(l.n_frames, l.n_bands), fft64::kLdsBytes<LOGN> + tap_lds, iq, l.cur, l.tw, l.psd, l.in_stride, l.frame_stride,
                   l.out_stride, l.n_frames, 1, tap.bins, tap.out, tap.n, tap.stride);
    } else {
        // the narrow formats' kernels: one frame per workgroup, always (FftChoice::frames_per_wg is the float32 kernel's)
        launch(one, dim3(l.n_frames, l.n_bands), fft64::kLdsBytes<LOGN> + tap_lds, static_cast<const typename IN::word *>(l.iq), l.cur, l.tw, l.psd,
               l.in_stride, l.frame_stride, l.out_stride, tap.bins, tap.out, tap.n, tap.stride);
    }
    return hipGetLastError();
}

// N = 512 - 16384: the kernels of fft_kernel(l.fft) for input format IN, windowed or plain; any other id refused
template <class IN, bool WIN>
hipError_t launch_fft_psd(const FftLaunch &l, LaunchAt at)
{
    switch (l.logn) {
    case 9: return launch_fft_t<IN, WIN, 9>(l, at);
    case 10: return launch_fft_t<IN, WIN, 10>(l, at);
    case 11: return launch_fft_t<IN, WIN, 11>(l, at);
    case 12: return launch_fft_t<IN, WIN, 12>(l, at);
    case 13: return launch_fft_t<IN, WIN, 13>(l, at);
    case 14: return launch_fft_t<IN, WIN, 14>(l, at);
    default: return hipErrorInvalidValue;
    }
}
// each instance lives in one unit (the file header); every other file that sees this header links to it
extern template hipError_t launch_fft_psd<InF32, false>(const FftLaunch &, LaunchAt);
extern template hipError_t launch_fft_psd<InSc16, false>(const FftLaunch &, LaunchAt);
extern template hipError_t launch_fft_psd<InF32, true>(const FftLaunch &, LaunchAt);
extern template hipError_t launch_fft_psd<InSc16, true>(const FftLaunch &, LaunchAt);
extern template hipError_t launch_fft_psd<InIq8, false>(const FftLaunch &, LaunchAt);
extern template hipError_t launch_fft_psd<InIq8, true>(const FftLaunch &, LaunchAt);

}  // namespace sdr
