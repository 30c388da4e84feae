// fft_2p.h — the two-phase radix-2 FFT of the block sizes whose float64 frame does not fit one CU (N = 32768, 65536).
//
// The radix-2 DIT FFT go-dsp runs (fft_f64.h) is a fixed butterfly graph over the bit-reversed input r[i] = x[brev(i)].
// Stages 1..A pair index bits 0..A-1: they act on the 2^B contiguous blocks r[k 2^A + m] (m < 2^A) one by one.  Stages
// A+1..A+B pair bits A..A+B-1: they act on the 2^A sets {c + 2^A q} (q < 2^B), one set per residue c.  So
//   phase A: sub-FFT k over m, input x[brev_A(m) 2^B + brev_B(k)], stages 1..A, written as the float64 intermediate
//            Y[k 2^A + m] (the DIT state behind stage A, in its natural order);
//   phase B: sub-FFT c over q, input Y[c + 2^A q], stages A+1..A+B; its outputs are the bins c + 2^A q.
// A stage s of either phase is go-dsp's: t = r[i + h] W[(N / 2h) j], j = i mod h, h = 2^(s-1), r[i] +- t, the complex
// multiply as (ac - bd, ad + bc), no contraction, the twiddle VALUES of go-dsp's table (uploaded once, unchanged).  In a
// phase-B set, j = c + 2^A (q mod 2^(s'-1)) at its local stage s' = s - A.  Same graph, same operations: the same bits.
//
// A sub-FFT of 2^MB points (MB = 7 or 8) is 2^(MB-4) threads x 16 points in registers, two register passes of radix-2
// stages: pass 0 holds index bits 0..3 in its register slots (local stages 1..4), pass 1 bits MB-4..MB-1 (stages 5..MB;
// at MB = 7 slot bit 0 holds bit 3, which pass 1 does not pair).  Between the passes one exchange through LDS.  A
// workgroup is 256 threads and holds G = 4096 / 2^MB sub-FFTs side by side; its lanes run across the sub-FFTs where that
// makes the global accesses contiguous (neighbouring samples in phase A's loads, neighbouring Y words in phase B's).
//
// Everything here is SDR_HD: tests/emu/emu_fft_2p.cpp runs these very functions thread by thread on the CPU.
#pragma once
#include <cstdint>

#include "fft_f64.h"
#include "sc16.h"

namespace fft2p {

using fft64::cplx;

constexpr int LOGR = 4, R = 1 << LOGR;  // points per thread
constexpr int T = 256;                  // threads per workgroup

// the split A + B of log N (phase A runs 2^A-point sub-FFTs, phase B 2^B-point ones)
template <int LOGN>
struct Split;
template <>
struct Split<15> {
    static constexpr int A = 8, B = 7;
};
template <>
struct Split<16> {
    static constexpr int A = 8, B = 8;
};

// a 2^MB-point sub-FFT as TPS threads x R points, G of them per workgroup
template <int MB>
struct Sub {
    static_assert(MB >= 5 && MB <= 8, "two register passes of at most four stages");
    static constexpr int M = 1 << MB;
    static constexpr int TPS = M / R;  // threads per sub-FFT
    static constexpr int G = T / TPS;  // sub-FFTs per workgroup
    static constexpr int P1 = MB - LOGR;  // pass 1's slots hold index bits P1 .. MB-1
    static constexpr int LDS_ROW = M + 1;  // doubles per sub-FFT row of the exchange area (+1: rows start in different banks)
    static constexpr int LDS_BYTES = 2 * G * LDS_ROW * 8;  // re and im
};

// Who holds what.  Pass 0: thread t works on sub-FFT t mod G and holds index m = slot | (t / G) << 4.  Pass 1 has two
// orders: LANES_M (phase A: consecutive lanes hold consecutive m, so Y is written in 256-byte runs) puts the sub-FFT in
// the high thread bits; otherwise (phase B: consecutive lanes hold consecutive residues c, so psd bins are neighbours)
// the low ones.  m = v | slot << P1 with v the thread's other part.
template <int MB>
SDR_HD inline int p0_sub(int t) { return t % Sub<MB>::G; }
template <int MB>
SDR_HD inline int p0_index(int t, int s) { return s | (t / Sub<MB>::G) << LOGR; }
template <int MB, bool LANES_M>
SDR_HD inline int p1_sub(int t) { return LANES_M ? t / Sub<MB>::TPS : t % Sub<MB>::G; }
template <int MB, bool LANES_M>
SDR_HD inline int p1_index(int t, int s)
{
    const int v = LANES_M ? t % Sub<MB>::TPS : t / Sub<MB>::G;
    return v | s << Sub<MB>::P1;
}

// One radix-2 stage on the thread's 16 points: slot bit `sbit` is the pair bit; `tw(s)` is the twiddle of the pair whose
// lower slot is s (it depends on the slot bits below sbit only, so it is fetched once per value of those).
template <class TW>
SDR_HD inline void stage(double (&xr)[R], double (&xi)[R], int sbit, TW tw)
{
    const int h = 1 << sbit;
    for (int lo = 0; lo < h; lo++) {
        const cplx w = tw(lo);
        for (int s = lo; s < R; s += 2 * h) {
            const int u = s + h;
            const double ar = xr[u], ai = xi[u];
            const double wr = ar * w.x - ai * w.y;
            const double wi = ar * w.y + ai * w.x;
            const double lr = xr[s], li = xi[s];
            xr[s] = lr + wr;
            xi[s] = li + wi;
            xr[u] = lr - wr;
            xi[u] = li - wi;
        }
    }
}

// go-dsp's twiddle index of local stage `st` of a sub-FFT at local index m (the pair's lower element): phase A
// (off = 0, c = 0) (N >> st) j; phase B (off = A) (N >> (st + A)) (c + (j << A)), j = m mod 2^(st-1)
SDR_HD inline int tw_index(int logn, int st, int off, int c, int m)
{
    const int j = m & ((1 << (st - 1)) - 1);
    return (c + (j << off)) << (logn - st - off);
}

// Pass 0 (local stages 1..4) of the sub-FFT at thread part u = t / G; `W(i)` reads go-dsp's table
template <int MB, class TwFn>
SDR_HD inline void pass0(double (&xr)[R], double (&xi)[R], int logn, int off, int c, int t, TwFn W)
{
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int sb = 0; sb < LOGR; sb++)
        stage(xr, xi, sb, [&](int lo) { return W(tw_index(logn, sb + 1, off, c, p0_index<MB>(t, lo))); });
}

// Pass 1 (local stages 5..MB): stage st pairs index bit st - 1 = slot bit st - 1 - P1
template <int MB, bool LANES_M, class TwFn>
SDR_HD inline void pass1(double (&xr)[R], double (&xi)[R], int logn, int off, int c, int t, TwFn W)
{
    constexpr int P1 = Sub<MB>::P1;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int st = LOGR + 1; st <= MB; st++) {
        const int sb = st - 1 - P1;
        stage(xr, xi, sb, [&](int lo) { return W(tw_index(logn, st, off, c, p1_index<MB, LANES_M>(t, lo))); });
    }
}

// Phase A's input sample for sub-FFT k = brev_B(p) at index m: x[brev_A(m) 2^B + p]
template <int LOGN>
SDR_HD inline int a_sample(int p, int m)
{
    return (int)fft64::brev_bits((unsigned)m, Split<LOGN>::A) << Split<LOGN>::B | p;
}
template <int LOGN>
SDR_HD inline int a_block(int p) { return (int)fft64::brev_bits((unsigned)p, Split<LOGN>::B); }

// Sub-FFTs (= values of p in phase A, residues c in phase B) per workgroup, and workgroups per frame
template <int LOGN>
struct Phases {
    static constexpr int N = 1 << LOGN, A = Split<LOGN>::A, B = Split<LOGN>::B;
    using SA = Sub<A>;
    using SB = Sub<B>;
    static constexpr int WG_A = (1 << B) / SA::G;  // phase A workgroups per frame
    static constexpr int WG_B = (1 << A) / SB::G;  // phase B workgroups per frame
    static constexpr int LDS_BYTES = SA::LDS_BYTES > SB::LDS_BYTES ? SA::LDS_BYTES : SB::LDS_BYTES;
    static_assert(WG_A * SA::G == (1 << B) && WG_B * SB::G == (1 << A), "whole workgroups per frame");
};

// psd of bin idx (the FFT's natural order) lands at spectrum index idx ^ N/2 (dsp/fft.go:54-57 fftshift)
SDR_HD inline float psd_of(double re, double im) { return (float)(re * re + im * im); }

}  // namespace fft2p
