// k_nb.hip — the impulse noise blanker's three passes (include/sdrainer_hip.h "impulse noise blanker", nb.h, host/nb_rule.h):
// memory-bound streams of small integers on the object's stream, in the manner of k_iq_sums.hip.
//
// A workgroup of either streaming pass owns a tile of 16 KB of consecutive raw bytes, which is always whole blocks (nb.h).
// Wave w owns bytes w * 4096 .. w * 4096 + 4095 of it as four rows of 1 KB: a lane reads 16 bytes per load and a wave's load
// is 1 KB of consecutive input.  A 16-byte group lies inside one block (a block is at least 64 bytes).
//
// k_nb_power_*   P[j] of the call's blocks: a group's sum of u^2 (udot4 for the byte formats: sum b^2 and sum b of the bytes
//                b = byte ^ flip, then u = a b + c as in host/iq_sums.h), a butterfly over the lanes that share a block, and
//                one LDS integer add per block and row (per wave where a block is 4 KB or more).  Integer sums: the bits
//                depend on no order.  Real and complex formats of one sample type are the same sum over all values.
// k_nb_gate<F>   a thread per block of the tile forms the block's threshold from the W powers in front of it (nb_threshold:
//                one shift per block, so a sample costs a 32-bit compare).  The `hold` samples in front of the tile are
//                judged again from the input, with their own block's threshold, and give the last impulse before the tile;
//                the call's first tile takes the open gate of the call before (NbTail) instead.  Impulse flags become the
//                gate by a max-scan of "position of the last impulse": within a lane's group, across the wave (shuffles),
//                down a wave's four rows, across the waves through LDS.  A lane writes its 16 bytes, blanked or copied; a
//                workgroup writes its two counts as one row of a slab; the last one saves the open gate.
// k_nb_carry     one workgroup: moves the last W powers to the front, also where the call had fewer than W blocks and old
//                ones survive, and adds the slab's rows to the record, of which it is the only writer (integer sums: exact).
//
// Static LDS: 2048 bytes (256 block sums of 8 bytes), 1080 bytes (257 thresholds, the lookback's and the four waves' last
// impulse, the four waves' two counts) and 16 bytes (the carry pass's two totals).  Nothing here needs more than 64 VGPRs:
// 16 hold a lane's four groups; eight waves per SIMD.
#include "nb.h"

namespace sdr {
namespace {

constexpr int kNbTileGroups = kNbTileBytes / 16;  // 1024
constexpr int kNbNone = -(1 << 30);               // "no impulse so far": any position minus this exceeds every hold

template <int FMT>
struct NbFmt {
    static constexpr int base = ddc_complex_base(FMT);
    static constexpr bool real = ddc_is_real(FMT);
    static constexpr int sb = ddc_sample_bytes(FMT);
    static constexpr int spg = 16 / sb;  // samples of a 16-byte group: 16, 8 or 4
    static_assert(nb_format(FMT), "an integer format");
};

__device__ __forceinline__ int nb_unit8(uint32_t byte, bool is_signed) { return is_signed ? (int)(signed char)byte : nb_unit_u8(byte); }

// m of sample e of a group (e is a constant once the loops are unrolled)
template <int FMT>
__device__ __forceinline__ uint32_t nb_mag(const uint32_t (&w)[4], int e)
{
    using F = NbFmt<FMT>;
    if constexpr (F::base == SDR_DDC_SC16 && F::real) {
        const int u = (int)(short)(w[e >> 1] >> (16 * (e & 1)));
        return (uint32_t)(u * u);
    } else if constexpr (F::base == SDR_DDC_SC16) {
        const int i = (int)(short)(w[e] & 0xffffu), q = (int)w[e] >> 16;
        return (uint32_t)(i * i) + (uint32_t)(q * q);  // (-32768, -32768): 2^31
    } else if constexpr (F::real) {
        const int u = nb_unit8((w[e >> 2] >> (8 * (e & 3))) & 0xffu, F::base == SDR_DDC_CS8);
        return (uint32_t)(u * u);
    } else {
        const uint32_t h = w[e >> 1] >> (16 * (e & 1));
        const int i = nb_unit8(h & 0xffu, F::base == SDR_DDC_CS8), q = nb_unit8((h >> 8) & 0xffu, F::base == SDR_DDC_CS8);
        return (uint32_t)(i * i + q * q);
    }
}

// the blank word over sample e of a group; a group starts on an even sample index, so k & 1 is e & 1
template <int FMT>
__device__ __forceinline__ void nb_blank(uint32_t (&w)[4], int e)
{
    using F = NbFmt<FMT>;
    const uint32_t par = (uint32_t)(e & 1);
    if constexpr (F::sb == 4) {
        w[e] = 0;
    } else if constexpr (F::sb == 2) {
        const uint32_t word = F::base == SDR_DDC_CU8 ? (127u + par) | ((128u - par) << 8) : 0u;
        w[e >> 1] = (w[e >> 1] & ~(0xffffu << (16 * (e & 1)))) | (word << (16 * (e & 1)));
    } else {
        const uint32_t word = F::base == SDR_DDC_CU8 ? 127u + par : 0u;
        w[e >> 2] = (w[e >> 2] & ~(0xffu << (8 * (e & 3)))) | (word << (8 * (e & 3)));
    }
}

// m of sample k of the input, one sample-sized load
template <int FMT>
__device__ __forceinline__ uint32_t nb_mag_at(const void *in, long long k)
{
    using F = NbFmt<FMT>;
    uint32_t w[4] = {0, 0, 0, 0};
    if constexpr (F::sb == 4)
        w[0] = static_cast<const uint32_t *>(in)[k];
    else if constexpr (F::sb == 2)
        w[0] = static_cast<const uint16_t *>(in)[k];
    else
        w[0] = static_cast<const uint8_t *>(in)[k];
    return nb_mag<FMT>(w, 0);
}

// -- the power pass ---------------------------------------------------------------------------------------------------------
// sum of u^2 over a group's values; BASE is the sample type (SDR_DDC_SC16, _CS8 or _CU8)
template <int BASE>
__device__ __forceinline__ unsigned long long nb_group_power(const uint4 &v)
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    if constexpr (BASE == SDR_DDC_SC16) {
        unsigned long long s = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int lo = (int)(short)(w[i] & 0xffffu), hi = (int)w[i] >> 16;
            s += (unsigned long long)(uint32_t)(lo * lo) + (uint32_t)(hi * hi);
        }
        return s;
    } else {
        constexpr uint32_t flip = BASE == SDR_DDC_CS8 ? 0x80808080u : 0u;
        constexpr int ua = BASE == SDR_DDC_CS8 ? 1 : 2, uc = BASE == SDR_DDC_CS8 ? -128 : -255;
        uint32_t s1 = 0, s2 = 0;  // 16 bytes: at most 4080 and 16 * 255^2
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t b = w[i] ^ flip;
            s1 = __builtin_amdgcn_udot4(b, 0x01010101u, s1, false);
            s2 = __builtin_amdgcn_udot4(b, b, s2, false);
        }
        return (unsigned long long)(ua * ua * (int)s2 + 2 * ua * uc * (int)s1 + 16 * uc * uc);  // sum (a b + c)^2 >= 0
    }
}

template <int BASE>
__global__ __launch_bounds__(kNbThreads) void k_nb_power(const uint4 *__restrict__ in, long long n_groups, int block_groups_log2,
                                                          unsigned long long *__restrict__ pow_call)
{
    __shared__ unsigned long long s_p[kNbTileBlocks];
    s_p[threadIdx.x] = 0;
    __syncthreads();
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int bgl = block_groups_log2;  // a block is 2^bgl groups, 4 .. 1024
    const int tg0 = wave * (kNbRows * 64) + lane;
    const long long g0 = (long long)blockIdx.x * kNbTileGroups + tg0;
    unsigned long long v[kNbRows];
#pragma unroll
    for (int r = 0; r < kNbRows; r++) {
        const long long g = g0 + r * 64;
        v[r] = g < n_groups ? nb_group_power<BASE>(in[g]) : 0ull;  // (the call ends on a block's end: a whole block or none)
    }
    if (bgl >= 8) {  // a block is a wave's 4 KB or more
        unsigned long long s = v[0] + v[1] + v[2] + v[3];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1)
            s += __shfl_xor(s, off, 64);
        if (lane == 0)
            atomicAdd(&s_p[tg0 >> bgl], s);
    } else {
        const int seg = bgl >= 6 ? 64 : 1 << bgl;  // lanes of a row that share a block
#pragma unroll
        for (int r = 0; r < kNbRows; r++) {
            unsigned long long s = v[r];
            for (int off = 1; off < seg; off <<= 1)
                s += __shfl_xor(s, off, 64);
            if ((lane & (seg - 1)) == 0)
                atomicAdd(&s_p[(tg0 + r * 64) >> bgl], s);
        }
    }
    __syncthreads();
    const int per_tile = kNbTileGroups >> bgl;
    const long long blk = (long long)blockIdx.x * per_tile + threadIdx.x, n_blocks = n_groups >> bgl;
    if ((int)threadIdx.x < per_tile && blk < n_blocks)
        pow_call[blk] = s_p[threadIdx.x];
}

// -- the gate pass ----------------------------------------------------------------------------------------------------------
struct NbGateArgs {
    long long n_groups;
    int block_groups_log2, window, span_log2, ratio_q4, hold, warm;
};

struct NbGateShared {
    uint32_t thr[kNbTileBlocks + 1];  // [0]: the block in front of the tile
    int look;                         // the last impulse among the `hold` samples in front of the tile (a negative position)
    int wave[kNbThreads / 64];        // each wave's last impulse
    unsigned count[kNbThreads / 64][2];  // each wave's impulses and blanked samples
};

template <int FMT>
__global__ __launch_bounds__(kNbThreads) void k_nb_gate(const uint4 *__restrict__ in, uint4 *__restrict__ out, NbGateArgs a,
                                                         const unsigned long long *__restrict__ pow, const NbTail *__restrict__ tail_in,
                                                         NbTail *__restrict__ tail_out, uint2 *__restrict__ part)
{
    using F = NbFmt<FMT>;
    __shared__ NbGateShared sh;
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int bgl = a.block_groups_log2, per_tile = kNbTileGroups >> bgl, hold = a.hold;
    const long long n_blocks = a.n_groups >> bgl, blk0 = (long long)blockIdx.x * per_tile;
    // positions are sample indices counted from the tile's first sample
    for (int i = t; i <= per_tile; i += kNbThreads) {
        const long long j = blk0 - 1 + i;  // the call's block j; its W powers in front are pow[j .. j + W - 1]
        uint32_t thr = kNbNever;
        if (j >= a.warm && j < n_blocks) {
            unsigned long long R = 0;
            for (int k = 0; k < a.window; k++)
                R += pow[j + k];
            thr = nb_threshold(R, a.ratio_q4, a.span_log2, true);
        }
        sh.thr[i] = thr;
    }
    if (t == 0)
        sh.look = kNbNone;
    __syncthreads();

    if (blockIdx.x > 0 && sh.thr[0] != kNbNever) {
        const long long s0 = (long long)blockIdx.x * (kNbTileGroups * F::spg);
        int best = kNbNone;
        for (int i = t; i < hold; i += kNbThreads)
            if (nb_over(nb_mag_at<FMT>(in, s0 - hold + i), sh.thr[0]))
                best = i - hold;
        if (best != kNbNone)
            atomicMax(&sh.look, best);
    }

    const int tg0 = wave * (kNbRows * 64) + lane;
    const long long g0 = (long long)blockIdx.x * kNbTileGroups + tg0;
    uint32_t w[kNbRows][4], flags[kNbRows];
    int before[kNbRows];  // the last impulse of this wave in front of the lane's group of row r
    int wave_last = kNbNone;
#pragma unroll
    for (int r = 0; r < kNbRows; r++) {
        const int tg = tg0 + r * 64;
        int last = kNbNone;
        flags[r] = 0;
        if (g0 + r * 64 < a.n_groups) {
            const uint4 v = in[g0 + r * 64];
            w[r][0] = v.x, w[r][1] = v.y, w[r][2] = v.z, w[r][3] = v.w;
            const uint32_t thr = sh.thr[1 + (tg >> bgl)];
#pragma unroll
            for (int e = 0; e < F::spg; e++)
                if (nb_over(nb_mag<FMT>(w[r], e), thr)) {
                    flags[r] |= 1u << e;
                    last = tg * F::spg + e;
                }
        }
        int incl = last;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int up = __shfl_up(incl, off, 64);
            if (lane >= off)
                incl = max(incl, up);
        }
        const int up = __shfl_up(incl, 1, 64);
        before[r] = max(wave_last, lane > 0 ? up : kNbNone);
        wave_last = max(wave_last, __shfl(incl, 63, 64));
    }
    if (lane == 0)
        sh.wave[wave] = wave_last;
    __syncthreads();

    int carry = sh.look;
    for (int i = 0; i < wave; i++)
        carry = max(carry, sh.wave[i]);
    const int open = blockIdx.x == 0 ? tail_in->open : 0;  // at most B samples: inside the call's first tile
    unsigned n_imp = 0, n_blank = 0;
#pragma unroll
    for (int r = 0; r < kNbRows; r++) {
        if (g0 + r * 64 >= a.n_groups)
            continue;
        const int p0 = (tg0 + r * 64) * F::spg;
        int prev = max(carry, before[r]);
        n_imp += (unsigned)__popc(flags[r]);
#pragma unroll
        for (int e = 0; e < F::spg; e++) {
            const int p = p0 + e;
            if (flags[r] & (1u << e))
                prev = p;
            if (p - prev <= hold || p < open) {
                nb_blank<FMT>(w[r], e);
                n_blank++;
            }
        }
        out[g0 + r * 64] = make_uint4(w[r][0], w[r][1], w[r][2], w[r][3]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_imp += __shfl_down(n_imp, off, 64);
        n_blank += __shfl_down(n_blank, off, 64);
    }
    if (lane == 0) {
        sh.count[wave][0] = n_imp;
        sh.count[wave][1] = n_blank;
    }
    __syncthreads();
    if (t == 0)  // one row per workgroup, summed by k_nb_carry: thousands of atomics on one line would outlast the stream
        part[blockIdx.x] = make_uint2(sh.count[0][0] + sh.count[1][0] + sh.count[2][0] + sh.count[3][0],
                                      sh.count[0][1] + sh.count[1][1] + sh.count[2][1] + sh.count[3][1]);
    if (blockIdx.x == gridDim.x - 1 && t == 0) {
        // the gate that runs into the next call: what is left of last + hold behind the call's last sample
        int last = sh.look;
        for (int i = 0; i < kNbThreads / 64; i++)
            last = max(last, sh.wave[i]);
        const int n_tile = (int)(a.n_groups - (long long)blockIdx.x * kNbTileGroups) * F::spg;
        tail_out->open = last == kNbNone ? 0 : max(0, last + hold - (n_tile - 1));
        tail_out->pad = 0;
    }
}

// -- the carry pass ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kNbThreads) void k_nb_carry(unsigned long long *__restrict__ pow, long long n_blocks, int window,
                                                          const uint2 *__restrict__ part, int tiles, unsigned long long *__restrict__ rec)
{
    __shared__ unsigned long long s_count[2];
    const int t = (int)threadIdx.x;
    const unsigned long long v = t < window ? pow[n_blocks + t] : 0ull;
    if (t < 2)
        s_count[t] = 0;
    __syncthreads();  // (a call of fewer than W blocks: source and destination overlap)
    if (t < window)
        pow[t] = v;
    // the call's two counts: the workgroups' rows, integer sums, and the record's one writer
    unsigned long long imp = 0, blank = 0;
    for (int i = t; i < tiles; i += kNbThreads) {
        const uint2 p = part[i];
        imp += p.x;
        blank += p.y;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        imp += __shfl_down(imp, off, 64);
        blank += __shfl_down(blank, off, 64);
    }
    if ((t & 63) == 0) {
        atomicAdd(&s_count[0], imp);
        atomicAdd(&s_count[1], blank);
    }
    __syncthreads();
    if (t < 2 && s_count[t])
        rec[t] += s_count[t];
}

template <int FMT>
void launch_gate(const NbLaunch &l, const NbGateArgs &a, unsigned tiles, hipStream_t stream)
{
    hipLaunchKernelGGL(k_nb_gate<FMT>, dim3(tiles), dim3(kNbThreads), 0, stream, static_cast<const uint4 *>(l.in), static_cast<uint4 *>(l.out), a,
                       l.pow, l.tail_in, l.tail_out, l.part);
}

}  // namespace

hipError_t launch_nb(const NbLaunch &l, hipStream_t stream)
{
    if (!nb_format(l.fmt) || !nb_geometry(l.block, l.window) || !nb_threshold_valid(l.block, l.ratio_q4, l.hold) || l.n <= 0 ||
        l.n % l.block != 0 || l.warm < 0)
        return hipErrorInvalidValue;
    const int sb = ddc_sample_bytes(l.fmt);
    const long long n_groups = l.n * sb / 16, n_blocks = l.n / l.block;
    const int bgl = nb_log2(l.block * sb / 16);
    const unsigned tiles = (unsigned)nb_tiles(l.fmt, l.n);
    const uint4 *in = static_cast<const uint4 *>(l.in);
    unsigned long long *pow_call = l.pow + l.window;
    switch (ddc_complex_base(l.fmt)) {
    case SDR_DDC_SC16:
        hipLaunchKernelGGL(k_nb_power<SDR_DDC_SC16>, dim3(tiles), dim3(kNbThreads), 0, stream, in, n_groups, bgl, pow_call);
        break;
    case SDR_DDC_CS8:
        hipLaunchKernelGGL(k_nb_power<SDR_DDC_CS8>, dim3(tiles), dim3(kNbThreads), 0, stream, in, n_groups, bgl, pow_call);
        break;
    default:
        hipLaunchKernelGGL(k_nb_power<SDR_DDC_CU8>, dim3(tiles), dim3(kNbThreads), 0, stream, in, n_groups, bgl, pow_call);
        break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    const NbGateArgs a{n_groups, bgl, l.window, nb_log2(l.block * l.window), l.ratio_q4, l.hold, l.warm};
    switch (l.fmt) {
    case SDR_DDC_SC16: launch_gate<SDR_DDC_SC16>(l, a, tiles, stream); break;
    case SDR_DDC_CS8: launch_gate<SDR_DDC_CS8>(l, a, tiles, stream); break;
    case SDR_DDC_CU8: launch_gate<SDR_DDC_CU8>(l, a, tiles, stream); break;
    case SDR_DDC_RS16: launch_gate<SDR_DDC_RS16>(l, a, tiles, stream); break;
    case SDR_DDC_RS8: launch_gate<SDR_DDC_RS8>(l, a, tiles, stream); break;
    default: launch_gate<SDR_DDC_RU8>(l, a, tiles, stream); break;
    }
    e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_nb_carry, dim3(1), dim3(kNbThreads), 0, stream, l.pow, n_blocks, l.window, l.part, (int)tiles, l.rec);
    return hipGetLastError();
}

}  // namespace sdr
