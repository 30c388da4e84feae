// fft_f64.h — register-tiled radix-2 DIT FFT in float64 whose arithmetic is *bit-identical* to the
// stage-by-stage radix-2 algorithm the reference calls (go-dsp fft.FFT, dsp/fft.go:26).
//
// Idea: a radix-2 decimation-in-time FFT is a fixed dataflow graph of butterflies
//     t = r[i+h] * W[(N/2h) * (i mod h)];  r[i] = r[i] + t;  r[i+h] = r[i] - t
// over a bit-reversed copy of the input.  Any schedule that evaluates that same graph with the same
// IEEE operations (complex multiply as (ac-bd, ad+bc), no FMA contraction) and the same twiddle
// VALUES produces the same bits.  So each thread keeps R = 16 (8 for N=512) points in VGPRs and runs
// LOGR consecutive stages on them (a "pass"), then the data is exchanged for the next pass.  One
// assignment of index bits to (register slot, lane, wave) per pass (make_layout) decides how: inside a
// wave's own block of LDS, across waves through LDS (once, behind pass 1), or - where only lane bits 4
// and 5 trade places with slot bits - in registers (make_swap_plan).  The frame itself is staged
// through LDS by LDS-DMA and read from there in pass 0's layout ("Input staging" below).  Twiddles are
// never recomputed on the device: the host builds go-dsp's table (radix2 factors via math.Sincos, even
// entries copied from the half-size table) and uploads it re-laid-out per pass so a wave reads them
// with coalesced 16-byte loads.
//
// Everything here is `SDR_HD` and free of HIP intrinsics so tests/emu can run the very same phase
// functions thread-by-thread on the CPU to validate the index math without a GPU.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SDR_HD __host__ __device__
#else
#define SDR_HD
#endif

namespace fft64 {

struct cplx {
    double x, y;
};

template <int LOGN>
struct Plan {
    static constexpr int N = 1 << LOGN;
    // points per thread: 16 for N >= 1024 (radix-16 register passes), 8 at N = 512.  (32 points at
    // N = 16384 would save an exchange, but its 31 twiddles per pass plus a prefetched frame spill.)
    static constexpr int LOGR = (LOGN >= 10) ? 4 : 3;
    static constexpr int R = 1 << LOGR;                       // points per thread
    static constexpr int T = N / R;                           // threads per frame
    static constexpr int LOGT = LOGN - LOGR;
    static constexpr int LOGL = 6;                            // lane bits of a thread id (64-wide waves)
    static constexpr int WB = LOGT - LOGL;                    // wave bits of a thread id
    static constexpr int NPASS = (LOGN + LOGR - 1) / LOGR;    // register passes
    static constexpr int LAST_LOG = LOGN - (NPASS - 1) * LOGR;
    static constexpr bool SPLIT = (N * 16 > 65536);           // exchange re / im separately through LDS
    // (bytes of LDS a frame needs: fft64::lds_bytes<LOGN>() - the exchange maps are padded, see make_addr)
    static_assert(LOGT >= LOGL, "a frame needs at least one full wave");

    SDR_HD static constexpr int pass_log(int p) { return p < NPASS - 1 ? LOGR : LAST_LOG; }
    // offset (in entries) of pass p's twiddle block: block p holds (2^pass_log(p) - 1) * R^p entries
    SDR_HD static constexpr int tw_offset(int p)
    {
        int o = 0;
        for (int k = 0; k < p; k++)
            o += ((1 << pass_log(k)) - 1) << (k * LOGR);
        return o;
    }
    static constexpr int TW_TOTAL = tw_offset(NPASS);
    // Exchange e (between pass e and e+1) moves data between waves only when the set of index bits
    // held in the wave id changes; that happens once, after pass 1 (see make_layout).  Every other
    // exchange stays inside a wave and needs no workgroup barrier.
    SDR_HD static constexpr bool cross_wave(int e) { return WB > 0 && e == 1; }
};

SDR_HD inline unsigned brev_bits(unsigned v, int bits)
{
    unsigned r = 0;
    for (int i = 0; i < bits; i++) {
        r = (r << 1) | (v & 1u);
        v >>= 1;
    }
    return r;
}

// ---------------------------------------------------------------------------------------------
// Who holds what.  During pass P the LOGN bits of an element's index i (in the bit-reversed work
// array) are spread over the register slot (LOGR bits), the lane (6 bits) and the wave (WB bits):
//
//   slot : the bits the pass's stages pair up, [4P, 4P+pass_log); a short last pass fills the slot
//          with the bits just below them
//   wave : passes 0,1: bits [8, 8+WB); later passes: the WB bits below the last pass's slot bits,
//          i.e. [8-WB, 8) (one lower when the last pass borrowed bit 7)
//   lane : everything else.  Pass 0 orders them downwards (lane bit 0 = top index bit = lowest
//          sample-number bit, so neighbouring lanes load neighbouring samples); later passes
//          upwards (lane bits 0-3 = index bits 0-3: coalesced twiddle loads and output stores).
//
// With that choice passes 0 and 1 share their wave bits, and so do passes 2 and 3: only the exchange
// after pass 1 crosses waves (Plan::cross_wave).  The exchanges that turn out to move nothing but lane
// bits 4 / 5 against slot bits need no LDS (make_swap_plan): exchange 1 at N = 1024 (no wave bits
// there), exchange 2 at N = 8192 and 16384.
// ---------------------------------------------------------------------------------------------
struct Layout {
    int sbit[4];   // index bit held by slot bit j
    int tbit[10];  // index bit held by thread-id bit j (lanes first, then waves)
};

template <int LOGN>
SDR_HD constexpr Layout make_layout(int P)
{
    using PL = Plan<LOGN>;
    Layout L{};
    bool used[16] = {};
    const int plog = PL::pass_log(P);
    const int base = P * PL::LOGR;
    for (int j = 0; j < PL::LOGR; j++) {
        L.sbit[j] = j < plog ? base + j : base - (PL::LOGR - plog) + (j - plog);
        used[L.sbit[j]] = true;
    }
    const int wz_hi = (PL::NPASS == 3) ? 2 * PL::LOGR - (PL::LOGR - PL::LAST_LOG) : 2 * PL::LOGR;
    const int wlo = (P <= 1) ? 2 * PL::LOGR : wz_hi - PL::WB;
    for (int j = 0; j < PL::WB; j++) {
        L.tbit[PL::LOGL + j] = wlo + j;
        used[wlo + j] = true;
    }
    int k = 0;
    if (P == 0) {
        for (int b = LOGN - 1; b >= 0; b--)
            if (!used[b])
                L.tbit[k++] = b;
    } else {
        for (int b = 0; b < LOGN; b++)
            if (!used[b])
                L.tbit[k++] = b;
    }
    return L;
}

// index bits contributed by the thread id / by the register slot during pass P
template <int LOGN, int P>
SDR_HD inline int thread_part(int t)
{
    constexpr Layout L = make_layout<LOGN>(P);
    int r = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < Plan<LOGN>::LOGT; j++)
        r |= ((t >> j) & 1) << L.tbit[j];
    return r;
}
template <int LOGN, int P>
SDR_HD constexpr int slot_part(int s)
{
    constexpr Layout L = make_layout<LOGN>(P);
    int r = 0;
    for (int j = 0; j < Plan<LOGN>::LOGR; j++)
        r |= ((s >> j) & 1) << L.sbit[j];
    return r;
}

// ---------------------------------------------------------------------------------------------
// Where a pass's twiddles sit in its table.  Pass P's twiddle for a butterfly depends on the index bits below
// the pass's own (lo = i mod 2^(P*LOGR)) and on the row (stage and position inside the register group).  Within a
// row the entries are stored in the order the THREADS want them: position bit 0 is the lowest of those index bits
// that sits in a lane, and so on through lanes, waves and (short last pass) the slot's spare bits - so that
// neighbouring lanes read neighbouring entries whatever the layout.
// ---------------------------------------------------------------------------------------------
struct TwPerm {
    int pos[16];  // index bit b (< P*LOGR) -> position bit
};

template <int LOGN>
SDR_HD constexpr TwPerm make_tw_perm(int P)
{
    using PL = Plan<LOGN>;
    const Layout L = make_layout<LOGN>(P);
    const int SH = P * PL::LOGR;
    TwPerm T{};
    int k = 0;
    for (int j = 0; j < PL::LOGT; j++)
        if (L.tbit[j] < SH)
            T.pos[L.tbit[j]] = k++;
    for (int j = 0; j < PL::LOGR; j++)
        if (L.sbit[j] < SH)
            T.pos[L.sbit[j]] = k++;
    return T;
}

// position of the entry for lo (host side, table construction)
template <int LOGN, int P>
SDR_HD constexpr int tw_pos_of_lo(int lo)
{
    constexpr TwPerm T = make_tw_perm<LOGN>(P);
    int r = 0;
    for (int b = 0; b < P * Plan<LOGN>::LOGR; b++)
        r |= ((lo >> b) & 1) << T.pos[b];
    return r;
}

// Index (in the bit-reversed work array r[]) of register slot (u, m) of thread t during pass P.
template <int LOGN, int P>
SDR_HD inline int elem_index(int t, int u, int m)
{
    return thread_part<LOGN, P>(t) | slot_part<LOGN, P>((u << Plan<LOGN>::pass_log(P)) + m);
}

// position (inside a row of pass P's twiddle table) of the entry thread t needs for register group u
template <int LOGN, int P>
SDR_HD inline int tw_pos(int t, int u)
{
    using PL = Plan<LOGN>;
    constexpr Layout L = make_layout<LOGN>(P);
    constexpr TwPerm T = make_tw_perm<LOGN>(P);
    constexpr int SH = P * PL::LOGR;
    int r = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < PL::LOGT; j++)
        if (L.tbit[j] < SH)
            r |= ((t >> j) & 1) << T.pos[L.tbit[j]];
    const int s = u << PL::pass_log(P);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < PL::LOGR; j++)
        if (L.sbit[j] < SH)
            r |= ((s >> j) & 1) << T.pos[L.sbit[j]];
    return r;
}

// ---------------------------------------------------------------------------------------------
// LDS address (in doubles) of index i during exchange E: a WEIGHTED SUM of the index bits, so that
// addr(thread_part | slot_part) = addr(thread_part) + addr(slot_part) and the slot half is a compile-time constant
// that goes into the DS instruction's offset field - one address register per side of an exchange (two where the
// constants pass 64 KB) instead of one per register slot (the XOR-swizzled map of rounds 1-2 cost the kernel about
// thirty address registers at the moment its register demand peaks).  The weights are chosen per exchange so that
// neither side has bank conflicts (MI355X: a ds_write_b64 is served in groups of 16 consecutive lanes over 32 banks,
// a ds_read_b64 in groups of 32 lanes over 64 banks), by padding rather than by swizzling:
//   the index bits in the reader's lane bits 0-4 get the weights 1, 2, 4, 8, 16 (32 lanes: 32 different words mod 32),
//     those that also sit in the writer's lane bits 0-3 first;
//   the remaining index bits of the writer's lane bits 0-3 get 32 * 2^j + (an unused one of 1, 2, 4, 8), so the
//     writer's 16 lanes fall on 16 different words mod 16 as well;
//   everything else is a multiple of the range those bits span, in this order: the writer's slot bits, the reader's
//     slot bits (small constants in the offset fields), the rest - and, in a wave-local exchange, the wave's bits last:
//     wave w then owns one contiguous block of words in every wave-local exchange, whichever index bits its id stands
//     for at the time, so consecutive wave-local exchanges need no barrier between them.
// ---------------------------------------------------------------------------------------------
struct AddrMap {
    int w[16];   // weight of index bit b, in doubles
    int size;    // words the exchange area spans
    int block;   // wave-local exchange: words per wave (0: cross-wave)
};

template <int LOGN>
SDR_HD constexpr AddrMap make_addr(int E)
{
    using PL = Plan<LOGN>;
    AddrMap A{};
    const Layout W = make_layout<LOGN>(E), Rd = make_layout<LOGN>(E + 1);
    bool used[16] = {};
    constexpr int NR = PL::LOGT < 5 ? PL::LOGT : 5;  // reader lane bits that share a ds_read_b64 group
    constexpr int NW = 4;                            // writer lane bits that share a ds_write_b64 group
    // 1. reader's low lane bits: powers of two, the ones shared with the writer's low lane bits first
    int k = 0;
    bool low_res_used[NW] = {};  // which of the residues 1, 2, 4, 8 (mod 16) the writer's lanes already have
    for (int pass = 0; pass < 2; pass++)
        for (int j = 0; j < NR; j++) {
            const int b = Rd.tbit[j];
            bool shared = false;
            for (int i = 0; i < NW; i++)
                shared = shared || (W.tbit[i] == b);
            if (used[b] || (pass == 0) != shared)
                continue;
            A.w[b] = 1 << k;
            if (shared && k < NW)
                low_res_used[k] = true;
            used[b] = true;
            k++;
        }
    int range = 1 << k;
    // 2. the writer's other low lane bits: 32 * 2^j plus an unused residue
    {
        int j = 0;
        for (int i = 0; i < NW; i++) {
            const int b = W.tbit[i];
            if (used[b])
                continue;
            int r = 0;
            while (r < NW && low_res_used[r])
                r++;
            low_res_used[r < NW ? r : NW - 1] = true;
            A.w[b] = ((1 << k) << j) + (1 << r);
            range = A.w[b] + range;  // (weights grow: the span so far is the sum of all weights + 1)
            used[b] = true;
            j++;
        }
    }
    // span of the bits placed so far = 1 + sum of their weights
    {
        int sum = 0;
        for (int b = 0; b < LOGN; b++)
            if (used[b])
                sum += A.w[b];
        range = sum + 1;
    }
    // 3. everything else: multiples of that range; writer's slot bits, reader's slot bits, the rest, wave bits last
    int mult = 1;
    auto place = [&](int b) {
        if (b < 0 || b >= LOGN || used[b])
            return;
        A.w[b] = range * mult;
        mult <<= 1;
        used[b] = true;
    };
    const bool local = !PL::cross_wave(E);
    bool is_wave[16] = {};
    if (local)
        for (int j = 0; j < PL::WB; j++)
            is_wave[W.tbit[PL::LOGL + j]] = true;
    for (int j = 0; j < PL::LOGR; j++)
        if (!is_wave[W.sbit[j]])
            place(W.sbit[j]);
    for (int j = 0; j < PL::LOGR; j++)
        if (!is_wave[Rd.sbit[j]])
            place(Rd.sbit[j]);
    for (int b = 0; b < LOGN; b++)
        if (!is_wave[b])
            place(b);
    A.block = local ? range * mult : 0;
    for (int j = 0; j < PL::WB; j++)
        if (local)
            place(W.tbit[PL::LOGL + j]);
    A.size = range * mult;
    return A;
}

template <int LOGN, int E>
SDR_HD constexpr int lds_addr(int i)
{
    constexpr AddrMap A = make_addr<LOGN>(E);
    int r = 0;
    for (int b = 0; b < LOGN; b++)
        r += ((i >> b) & 1) * A.w[b];
    return r;
}

// the same for the thread's part of an index during pass P (run-time argument: unrolled over the thread-id bits, the
// weights become literals)
template <int LOGN, int E, int P>
SDR_HD inline int lds_addr_thread(int t)
{
    constexpr AddrMap A = make_addr<LOGN>(E);
    constexpr Layout L = make_layout<LOGN>(P);
    int r = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int j = 0; j < Plan<LOGN>::LOGT; j++)
        r += ((t >> j) & 1) * A.w[L.tbit[j]];
    return r;
}

// words the exchanges of a frame need (the largest of the LDS exchanges' spans)
template <int LOGN>
SDR_HD constexpr int exchange_words()
{
    using PL = Plan<LOGN>;
    int m = PL::N;
    for (int e = 0; e < PL::NPASS - 1; e++) {
        const int sz = make_addr<LOGN>(e).size;
        m = sz > m ? sz : m;
    }
    return m;
}

// (as variables: a constexpr FUNCTION called where a constant is not required may be compiled and called at run time)
template <int LOGN>
inline constexpr int kExchangeWords = exchange_words<LOGN>();
template <int LOGN>
inline constexpr int kLdsBytes = (Plan<LOGN>::SPLIT ? 1 : 2) * kExchangeWords<LOGN> * 8;
template <int LOGN>
SDR_HD constexpr int lds_bytes()
{
    return kLdsBytes<LOGN>;
}

// ---------------------------------------------------------------------------------------------
// Register exchange.  When exchange E only trades slot bits for the index bits held in lane bits 4
// and 5 (everything else stays where it is), it needs no LDS at all: gfx950's v_permlane16_swap /
// v_permlane32_swap exchange the upper half-rows / upper half of one register with the lower ones of
// another, which IS the swap of a register-index bit with lane bit 4 / 5.  64 VALU instructions per
// wave for the last exchange at N = 16384 instead of 64 LDS instructions, four dependent LDS round
// trips and a barrier.
// ---------------------------------------------------------------------------------------------
struct SwapPlan {
    bool ok;
    int slot_bit_lane4;  // slot bit that trades places with lane bit 4 (-1: lane bit 4 keeps its index bit)
    int slot_bit_lane5;
};

template <int LOGN>
SDR_HD constexpr SwapPlan make_swap_plan(int E)
{
    using PL = Plan<LOGN>;
    const Layout A = make_layout<LOGN>(E), B = make_layout<LOGN>(E + 1);
    SwapPlan p{true, -1, -1};
    for (int j = 0; j < PL::LOGT; j++)
        if (j != 4 && j != 5 && A.tbit[j] != B.tbit[j])
            p.ok = false;
    for (int j = 0; j < PL::LOGR; j++) {
        if (A.sbit[j] == B.sbit[j])
            continue;
        if (B.sbit[j] == A.tbit[4] && A.sbit[j] == B.tbit[4] && p.slot_bit_lane4 < 0)
            p.slot_bit_lane4 = j;
        else if (B.sbit[j] == A.tbit[5] && A.sbit[j] == B.tbit[5] && p.slot_bit_lane5 < 0)
            p.slot_bit_lane5 = j;
        else
            p.ok = false;
    }
    if (p.slot_bit_lane4 < 0 && A.tbit[4] != B.tbit[4])
        p.ok = false;
    if (p.slot_bit_lane5 < 0 && A.tbit[5] != B.tbit[5])
        p.ok = false;
    if (p.slot_bit_lane4 < 0 && p.slot_bit_lane5 < 0)
        p.ok = false;
#if defined(SDR_FFT_NO_SWAP)
    p.ok = false;  // diagnostic builds: every exchange through LDS
#endif
    return p;
}

// Host-side model of the same exchange for one wave (x[lane][slot]); tests/emu uses it.
template <int LOGN, int E>
inline void exchange_swap_wave(double (*x)[Plan<LOGN>::R])
{
    constexpr SwapPlan P = make_swap_plan<LOGN>(E);
    static_assert(P.ok, "exchange is not a register swap");
    for (int round = 0; round < 2; round++) {
        const int sb = round == 0 ? P.slot_bit_lane4 : P.slot_bit_lane5;
        const int half = round == 0 ? 16 : 32;
        if (sb < 0)
            continue;
        for (int a = 0; a < Plan<LOGN>::R; a++) {
            if ((a >> sb) & 1)
                continue;
            const int b = a | (1 << sb);
            // v_permlaneNN_swap A, B: A's lanes with the bit set <-> B's lanes with the bit clear
            for (int l = 0; l < 64; l++)
                if (!(l & half)) {
                    const double t = x[l + half][a];
                    x[l + half][a] = x[l][b];
                    x[l][b] = t;
                }
        }
    }
}

#if defined(__HIPCC__)
__device__ __forceinline__ void swap_halves(double &a, double &b, bool rows16)
{
    unsigned alo = (unsigned)__double2loint(a), ahi = (unsigned)__double2hiint(a);
    unsigned blo = (unsigned)__double2loint(b), bhi = (unsigned)__double2hiint(b);
    if (rows16) {
        const auto lo = __builtin_amdgcn_permlane16_swap(alo, blo, false, false);
        const auto hi = __builtin_amdgcn_permlane16_swap(ahi, bhi, false, false);
        alo = lo[0], blo = lo[1], ahi = hi[0], bhi = hi[1];
    } else {
        const auto lo = __builtin_amdgcn_permlane32_swap(alo, blo, false, false);
        const auto hi = __builtin_amdgcn_permlane32_swap(ahi, bhi, false, false);
        alo = lo[0], blo = lo[1], ahi = hi[0], bhi = hi[1];
    }
    a = __hiloint2double((int)ahi, (int)alo);
    b = __hiloint2double((int)bhi, (int)blo);
}

template <int LOGN, int E>
__device__ __forceinline__ void exchange_swap(double (&x)[Plan<LOGN>::R])
{
    constexpr SwapPlan P = make_swap_plan<LOGN>(E);
    static_assert(P.ok, "exchange is not a register swap");
#pragma unroll
    for (int a = 0; a < Plan<LOGN>::R; a++)
        if (P.slot_bit_lane4 >= 0 && !((a >> P.slot_bit_lane4) & 1))
            swap_halves(x[a], x[a | (1 << P.slot_bit_lane4)], true);
#pragma unroll
    for (int a = 0; a < Plan<LOGN>::R; a++)
        if (P.slot_bit_lane5 >= 0 && !((a >> P.slot_bit_lane5) & 1))
            swap_halves(x[a], x[a | (1 << P.slot_bit_lane5)], false);
}
#endif

// Sample number (natural order) held in slot m of thread t at the start of pass 0.
template <int LOGN>
SDR_HD inline int input_sample(int t, int m)
{
    return (int)brev_bits((unsigned)elem_index<LOGN, 0>(t, 0, m), LOGN);
}

// ---------------------------------------------------------------------------------------------
// Input staging through LDS.  Pass 0 wants lane neighbours 32 bytes apart in memory at best (make_layout),
// which costs the texture unit four times the cache-line look-ups of a contiguous read.  So the frame is
// first copied global -> LDS by LDS-DMA (global_load_lds_dwordx4: no registers, each wave instruction one
// contiguous 1 KB row) and then read from LDS in the pass-0 layout.  LDS-DMA writes lane l's 16 bytes at row
// base + 16*l, so the image is shaped through the SOURCE address: lane p of row r fetches granule
// g = granule(p, r) (a granule = 16 bytes = 2^LOGS samples); the XOR swizzle spreads the rows and row parts that
// the 32 lanes of an LDS read group touch over the LDS banks.
//   sample n  ->  row r = n >> (6 + LOGS), granule g = (n >> LOGS) & 63,
//                 byte address r*1024 + pos(g, r)*16 + (n & (2^LOGS - 1)) * (16 >> LOGS)
// One image per input format, InImage<LOGN, LOGS, RULE>: float32 here (LOGS = 1: 128 samples per row, read with
// ds_read_b64, 32 lanes over 32 eight-byte bank pairs), sc16.h (LOGS = 2) and iq8.h (LOGS = 3), each with what its reads
// need from the banks.  RULE::make() says which bit each of three position bits is XORed with.
// ---------------------------------------------------------------------------------------------
struct InSwz {
    int first;   // the swizzled position bits are first, first + 1, first + 2
    int src[3];  // position bit first + k is XORed with: -1 nothing, 0..5 granule bit, 8+j row bit j
};

// The rule of the float32 and sc16 images.  Pass 0's lane bits 0 and 1 are sample bits 0 and 1, which lie inside the
// granule or (float32: sample bit 1) on position bit 0; position bit first + k pairs with lane bit 2 + k and is XORed
// with the sample bit behind it, unless that is the bit a linear image has there.
template <int LOGN, int LOGS>
struct PairedSwz {
    static_assert(LOGS == 1 || LOGS == 2, "sample bits 0 and 1 must end below position bit `first`");
    SDR_HD static constexpr InSwz make()
    {
        const Layout L0 = make_layout<LOGN>(0);
        InSwz z{2 - LOGS, {-1, -1, -1}};
        for (int k = 0; k < 3; k++) {
            const int nb = LOGN - 1 - L0.tbit[2 + k];  // sample-number bit behind lane bit 2+k
            if (nb >= 6 + LOGS)
                z.src[k] = 8 + (nb - (6 + LOGS));
            else if (nb - LOGS != z.first + k)
                z.src[k] = nb - LOGS;
        }
        return z;
    }
};

template <int LOGN, int LOGS, class RULE = PairedSwz<LOGN, LOGS>>
struct InImage {
    static constexpr int SAMPLE_BYTES = 16 >> LOGS;
    static constexpr int ROW_SAMPLES = 64 << LOGS;                // one 1 KB row
    static constexpr int ROWS = (1 << LOGN) / ROW_SAMPLES;        // of the image
    static constexpr int ROWS_PER_WAVE = Plan<LOGN>::R >> LOGS;   // each wave of the workgroup fetches (N = 512: one wave)
    static_assert(ROWS_PER_WAVE >= 1 && ROWS_PER_WAVE * (Plan<LOGN>::T / 64) == ROWS, "the waves' rows cover the frame exactly");

    SDR_HD static constexpr bool solvable()
    {
        const InSwz z = RULE::make();
        for (int k = 0; k < 3; k++)
            if (z.src[k] >= 0 && z.src[k] < 8 && z.src[k] <= z.first + k)
                return false;  // a position bit may only depend on higher granule bits (granule() solves downwards)
        return true;
    }

    SDR_HD static inline int pos(int g, int r)
    {
        constexpr InSwz Z = RULE::make();
        int p = g;
        for (int k = 0; k < 3; k++) {
            if (Z.src[k] >= 8)
                p ^= ((r >> (Z.src[k] - 8)) & 1) << (Z.first + k);
            else if (Z.src[k] >= 0)
                p ^= ((g >> Z.src[k]) & 1) << (Z.first + k);
        }
        return p;
    }

    // the granule lane p of row r fetches (the inverse of pos)
    SDR_HD static inline int granule(int p, int r)
    {
        static_assert(solvable(), "input swizzle is not triangular");
        constexpr InSwz Z = RULE::make();
        int g = p;
        for (int k = 2; k >= 0; k--) {
            if (Z.src[k] >= 8)
                g ^= ((r >> (Z.src[k] - 8)) & 1) << (Z.first + k);
            else if (Z.src[k] >= 0)
                g ^= ((g >> Z.src[k]) & 1) << (Z.first + k);  // bit src[k] > first + k is final already
        }
        return g;
    }

    // byte address of sample n in the image (linear over GF(2): thread and slot parts of n combine by XOR)
    SDR_HD static inline int lds_byte(int n)
    {
        const int r = n >> (6 + LOGS), g = (n >> LOGS) & 63;
        return r * 1024 + pos(g, r) * 16 + (n & ((1 << LOGS) - 1)) * SAMPLE_BYTES;
    }
};
template <int LOGN>
using InImageF32 = InImage<LOGN, 1>;
// the float32 image's functions by the names tests/emu audits them under
template <int LOGN>
SDR_HD inline int in_granule(int p, int r) { return InImageF32<LOGN>::granule(p, r); }
template <int LOGN>
SDR_HD inline int in_lds_byte(int n) { return InImageF32<LOGN>::lds_byte(n); }

// Pass 0 input: slot m <- x[input_sample(t, m)], widened to float64
// (dsp/fft.go:59-69 setSamplesFromIQ).
template <int LOGN>
SDR_HD inline void load_input(const float *iq, int t, double *xr, double *xi)
{
    using PL = Plan<LOGN>;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int m = 0; m < PL::R; m++) {
        const int n = input_sample<LOGN>(t, m);
        xr[m] = (double)iq[2 * n];
        xi[m] = (double)iq[2 * n + 1];
    }
}

// Pass P: pass_log(P) radix-2 stages on the thread's registers.  `tw_at(c, lo)` returns twiddle table
// entry c + lo, where c (the row) is a compile-time constant and lo = tw_pos(t, u) the only per-thread part (the
// kernel turns that split into a buffer load with c in the scalar offset; the emulator indexes an array).
// stage Q of pass P on register group u (compile-time loop over the stages: every bound below is a constant
// expression, so the twiddle arrays and the data stay in registers)
template <int LOGN, int P, int Q, class TW>
SDR_HD inline void butterfly_stages(double *xr, double *xi, int u, int lo, TW &tw_at)
{
    using PL = Plan<LOGN>;
    constexpr int PLOG = PL::pass_log(P);
    if constexpr (Q < PLOG) {
        constexpr int RP = 1 << PLOG;
        constexpr int S = 1 << (P * PL::LOGR);
        constexpr int OFF = PL::tw_offset(P);
        constexpr int ROWS = 1 << Q;
        double wr[ROWS], wi[ROWS];
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int mm = 0; mm < ROWS; mm++) {
            // pass 0 has thread-independent twiddles; W[0] = 1 and W[N/4] = -i are the literal
            // entries of go-dsp's size-4 table, multiplying by them is exact (up to the sign of a
            // zero, which cannot reach |X|^2), so the multiply is skipped.
            const bool one = (P == 0 && mm == 0);
            const bool minus_i = (P == 0 && Q >= 1 && mm == (ROWS >> 1));
            wr[mm] = 1.0;
            wi[mm] = 0.0;
            if (!one && !minus_i) {
#if defined(SDR_ABLATE) && (SDR_ABLATE == 3)
                wr[mm] = 0.5 + 1e-9 * lo;  // timing-only build: no twiddle loads
                wi[mm] = 0.25;
#else
                const cplx w = tw_at(OFF + (ROWS - 1 + mm) * S, lo);
                wr[mm] = w.x;
                wi[mm] = w.y;
#endif
            }
        }
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int mm = 0; mm < ROWS; mm++) {
            const bool one = (P == 0 && mm == 0);
            const bool minus_i = (P == 0 && Q >= 1 && mm == (ROWS >> 1));
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int k = 0; k < (RP >> (Q + 1)); k++) {
                const int a = u * RP + mm + (k << (Q + 1));
                const int b = a + ROWS;
                double tr, ti;
                if (one) {
                    tr = xr[b];
                    ti = xi[b];
                } else if (minus_i) {
                    tr = xi[b];
                    ti = -xr[b];
                } else {
                    tr = xr[b] * wr[mm] - xi[b] * wi[mm];  // Go complex128 multiply, amd64: no FMA
                    ti = xr[b] * wi[mm] + xi[b] * wr[mm];
                }
                const double ar = xr[a], ai = xi[a];
                xr[a] = ar + tr;
                xi[a] = ai + ti;
                xr[b] = ar - tr;
                xi[b] = ai - ti;
            }
        }
        butterfly_stages<LOGN, P, Q + 1>(xr, xi, u, lo, tw_at);
    }
}

template <int LOGN, int P, class TW>
SDR_HD inline void butterfly_pass(double *xr, double *xi, int t, TW tw_at)
{
    using PL = Plan<LOGN>;
    constexpr int G = PL::R >> PL::pass_log(P);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int u = 0; u < G; u++) {
        const int lo = (P == 0) ? 0 : tw_pos<LOGN, P>(t, u);  // position inside the row, see make_tw_perm
        butterfly_stages<LOGN, P, 0>(xr, xi, u, lo, tw_at);
    }
}

// Exchange E, write side: scatter the thread's slots (pass E layout) into LDS.
template <int LOGN, int E>
SDR_HD inline void exchange_write(const double *x, int t, double *lds)
{
    using PL = Plan<LOGN>;
    const int base = lds_addr_thread<LOGN, E, E>(t);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int s = 0; s < PL::R; s++)
        lds[base + lds_addr<LOGN, E>(slot_part<LOGN, E>(s))] = x[s];
}

// Exchange E, read side: gather the slots of pass E+1.
template <int LOGN, int E>
SDR_HD inline void exchange_read(double *x, int t, const double *lds)
{
    using PL = Plan<LOGN>;
    const int base = lds_addr_thread<LOGN, E, E + 1>(t);
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int s = 0; s < PL::R; s++)
        x[s] = lds[base + lds_addr<LOGN, E>(slot_part<LOGN, E + 1>(s))];
}

// Natural-order DFT bin held in register slot s = u*RP+m after the last pass.
template <int LOGN>
SDR_HD inline int output_bin(int t, int s)
{
    using PL = Plan<LOGN>;
    constexpr int RP = 1 << PL::LAST_LOG;
    return elem_index<LOGN, PL::NPASS - 1>(t, s / RP, s % RP);
}

// (host only)
// Host: lay go-dsp's factor table W[k] = e^{-2 pi i k / N} (k < N) out per pass:
// entry OFF_p + ((2^q - 1) + mm) * S_p + pos_p(lo)  =  W[(N / (2 * S_p * 2^q)) * (mm * S_p + lo)]
// (pos_p: the order the threads of pass p read a row in, make_tw_perm).
template <int LOGN, int P>
inline void build_one_pass_twiddles(const double *wre, const double *wim, cplx *out)
{
    using PL = Plan<LOGN>;
    if constexpr (P < PL::NPASS) {
        const int S = 1 << (P * PL::LOGR);
        const int off = PL::tw_offset(P);
        for (int q = 0; q < PL::pass_log(P); q++)
            for (int mm = 0; mm < (1 << q); mm++)
                for (int lo = 0; lo < S; lo++) {
                    const int h = S << q;
                    const int k = (PL::N / (2 * h)) * (mm * S + lo);
                    out[off + ((1 << q) - 1 + mm) * S + tw_pos_of_lo<LOGN, P>(lo)] = cplx{wre[k], wim[k]};
                }
        build_one_pass_twiddles<LOGN, P + 1>(wre, wim, out);
    }
}
template <int LOGN>
inline void build_pass_twiddles(const double *wre, const double *wim, cplx *out)
{
    build_one_pass_twiddles<LOGN, 0>(wre, wim, out);
}

}  // namespace fft64
