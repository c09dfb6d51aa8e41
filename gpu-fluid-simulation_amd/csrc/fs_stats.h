// fs_stats.h — the device helpers the two diagnostics kernels share (kernels_stats.hip k_stats and k_stats_fold, kernels_stats3d.hip
// k3_stats; include/fluidsim.h "fluid diagnostics"): the order-preserving key of a float, the per-lane accumulator
// of a record and of a channel value, the block's reduction into its row of the partials slab, and the fold of the slab into the
// fs_stats / fs3_stats record.  D is the number of components (2 or 3).  Device code only; the constants are fs_kernels.h's.
#pragma once
#include <hip/hip_runtime.h>

#include "fs_body_loads.h"

namespace fsd {

static_assert(STATS_SHIFT == BODY_LOAD_SHIFT, "Q is the body loads' Q");

// A row of the slab, 64-bit words.  First the words that are added: the 2D + 2 sums in the record's order (momentum, energy,
// position, density), nonfinite, dropped, attr_q[4], attr_dropped[4].  Then the keys, one per word, reduced with an unsigned
// maximum: speed2_max, density_min, density_max, pos_min[D], pos_max[D], attr_min[4], attr_max[4] — a minimum is kept as the
// complement of its key, so that one reduction serves both.
constexpr int stats_sums(int D) { return 2 * D + 2; }
constexpr int stats_sum_words(int D) { return stats_sums(D) + 10; }
constexpr int stats_keys(int D) { return 3 + 2 * D; }                   // of the record; eight channel keys follow
static_assert(stats_sum_words(2) + stats_keys(2) + 8 == (int)stats_words(2) && stats_sum_words(3) + stats_keys(3) + 8 == (int)stats_words(3),
              "fs_kernels.h stats_words");
constexpr bool stats_key_is_min(int D, int k) { return k == 1 || (k >= 3 && k < 3 + D) || (k >= stats_keys(D) && k < stats_keys(D) + 4); }
// Where word w of a row lands in fs_stats (D = 2) / fs3_stats (D = 3): byte offsets (engine_stats.hip and engine_3d_stats.hip
// assert them against offsetof).  count is at 0; tick, channels and pad at stats_attr_offset - 4, + 96 and + 100.
constexpr int stats_attr_offset(int D) { return 24 + 8 * stats_sums(D) + 4 * stats_keys(D) + 4; }      // attr_q
constexpr int stats_word_offset(int D, int w) {
    return w < stats_sums(D)            ? 24 + 8 * w
           : w < stats_sums(D) + 2      ? 8 + 8 * (w - stats_sums(D))                                   // nonfinite, dropped
           : w < stats_sum_words(D)     ? stats_attr_offset(D) + 8 * (w - stats_sums(D) - 2)            // attr_q, attr_dropped
           : w < stats_sum_words(D) + stats_keys(D) ? 24 + 8 * stats_sums(D) + 4 * (w - stats_sum_words(D))
                                        : stats_attr_offset(D) + 64 + 4 * (w - stats_sum_words(D) - stats_keys(D));   // attr_min, attr_max
}

// The usual order-preserving map of a non-NaN float to u32: -inf < ... < -0 < +0 < ... < +inf.  STATS_KEY_NONE is the key of -inf
// and the complement of the key of +inf: where every maximum and every (complemented) minimum starts.
constexpr uint32_t STATS_KEY_NONE = 0x007fffffu;
constexpr uint32_t STATS_BITS_INF = 0x7f800000u;        // |x| as bits: >= is NaN or inf
constexpr uint32_t STATS_BITS_LIMIT = 0x46800000u;      // 16384.0f: in(x) is |x| as bits < this
__device__ __forceinline__ uint32_t stats_key(float x) {
    const uint32_t b = __float_as_uint(x);
    return b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ float stats_unkey(uint32_t k) { return __uint_as_float(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xffffffffu)); }
__device__ __forceinline__ uint32_t stats_abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// Q(x) as a double, for a lane's running sum: x * 2^20 is exact in f32 for |x| < 2^14, rintf rounds ties to even, and a lane adds
// fewer than 2^19 values below 2^34, so the f64 sum is exact and converts to the integer once, after the loop.
__device__ __forceinline__ double stats_q(float x) { return (double)rintf(x * (float)(1u << STATS_SHIFT)); }

// max(v, v of the lane SHR places below in the row of 16; 0 where that leaves the row): the row form of wave_sum's step
template <int SHR>
__device__ __forceinline__ uint32_t row_shr_umax(uint32_t v) {
    return umax(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x110 + SHR, 0xf, 0xf, true));
}
// The unsigned maximum over the wave's 64 lanes, wave-uniform (all lanes active).
__device__ __forceinline__ uint32_t wave_umax(uint32_t v) {
    v = row_shr_umax<1>(v); v = row_shr_umax<2>(v); v = row_shr_umax<4>(v); v = row_shr_umax<8>(v);
    uint32_t m = 0u;
    for (int r = 15; r < 64; r += 16) m = umax(m, (uint32_t)__builtin_amdgcn_readlane((int)v, r));
    return m;
}

// What a lane keeps in registers over the whole loop.
template <int D>
struct StatsAcc {
    double s[stats_sums(D)];
    uint32_t nonfinite, dropped;
    uint32_t k[stats_keys(D)];
    double aq[4];
    uint32_t adrop[4];
    uint32_t ak[8];                  // ~min keys, then max keys
    __device__ __forceinline__ void init() {
        for (double& x : s) x = 0.0;
        nonfinite = dropped = 0u;
        for (uint32_t& x : k) x = STATS_KEY_NONE;
        for (double& x : aq) x = 0.0;
        for (uint32_t& x : adrop) x = 0u;
        for (uint32_t& x : ak) x = STATS_KEY_NONE;
    }
};

// One record: the header's "per record i".
template <int D>
__device__ __forceinline__ void stats_record(StatsAcc<D>& A, const float (&p)[D], const float (&v)[D], float rho) {
    uint32_t m = stats_abs_bits(rho);
#pragma unroll
    for (int a = 0; a < D; ++a) m = umax(m, umax(stats_abs_bits(p[a]), stats_abs_bits(v[a])));
    if (m >= STATS_BITS_INF) {
        A.nonfinite += 1u;
    } else {
        float e = __fadd_rn(__fmul_rn(v[0], v[0]), __fmul_rn(v[1], v[1]));
        if (D == 3) e = __fadd_rn(e, __fmul_rn(v[D - 1], v[D - 1]));
        A.k[0] = umax(A.k[0], stats_key(e));
        const uint32_t kr = stats_key(rho);
        A.k[1] = umax(A.k[1], ~kr);
        A.k[2] = umax(A.k[2], kr);
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const uint32_t kp = stats_key(p[a]);
            A.k[3 + a] = umax(A.k[3 + a], ~kp);
            A.k[3 + D + a] = umax(A.k[3 + D + a], kp);
        }
        if (umax(m, __float_as_uint(e)) < STATS_BITS_LIMIT) {     // e is +0 or above: its bits order as its value, +inf fails
#pragma unroll
            for (int a = 0; a < D; ++a) {
                A.s[a] += stats_q(v[a]);
                A.s[D + 1 + a] += stats_q(p[a]);
            }
            A.s[D] += stats_q(e);
            A.s[2 * D + 1] += stats_q(rho);
        } else {
            A.dropped += 1u;
        }
    }
}

// One value of channel c: the header's "per tracking channel".
template <int D>
__device__ __forceinline__ void stats_attr(StatsAcc<D>& A, int c, float a) {
    const uint32_t m = stats_abs_bits(a);
    if (m >= STATS_BITS_INF) {
        A.adrop[c] += 1u;
    } else {
        const uint32_t k = stats_key(a);
        A.ak[c] = umax(A.ak[c], ~k);
        A.ak[4 + c] = umax(A.ak[4 + c], k);
        if (m < STATS_BITS_LIMIT) A.aq[c] += stats_q(a);
        else A.adrop[c] += 1u;
    }
}

// Once per block of STATS_THREADS lanes, all of them active: the DPP reductions of every word over each wave, the four waves
// through LDS, one plain store of the block's words into its row of the slab.
template <int D>
__device__ __forceinline__ void stats_block_store(const StatsAcc<D>& A, u64* __restrict__ row) {
    constexpr int NS = stats_sums(D), SUMW = stats_sum_words(D), NK = stats_keys(D), WORDS = (int)stats_words(D);
    static_assert(STATS_THREADS == 256u && WORDS <= 64, "four waves; the first wave stores the row");
    __shared__ u64 part[4][WORDS];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    long long w[SUMW];
#pragma unroll
    for (int i = 0; i < NS; ++i) w[i] = (long long)A.s[i];
    w[NS] = (long long)A.nonfinite; w[NS + 1] = (long long)A.dropped;
#pragma unroll
    for (int c = 0; c < 4; ++c) { w[NS + 2 + c] = (long long)A.aq[c]; w[NS + 6 + c] = (long long)A.adrop[c]; }
#pragma unroll
    for (int i = 0; i < SUMW; ++i) {
        const long long r = wave_sum(w[i]);
        if (lane == 0u) part[wave][i] = (u64)r;
    }
#pragma unroll
    for (int i = 0; i < NK + 8; ++i) {
        const uint32_t r = wave_umax(i < NK ? A.k[i] : A.ak[i - NK]);
        if (lane == 0u) part[wave][SUMW + i] = (u64)r;
    }
    __syncthreads();
    const uint32_t t = threadIdx.x;
    if (t < (uint32_t)WORDS) {
        const u64 a = part[0][t], b = part[1][t], c = part[2][t], d = part[3][t];
        const u64 ab = a > b ? a : b, cd = c > d ? c : d;
        row[t] = t < (uint32_t)SUMW ? (a + b) + (c + d) : (ab > cd ? ab : cd);
    }
}

// k_stats_fold's body: block w (one wave) owns word w of the rows.  Lanes stride over the rows, the wave reduces, lane 0 turns a
// key back into its float and stores the field; block 0 also stores what the host knows: count, tick, channels, pad.
template <int D>
__device__ __forceinline__ void stats_fold(const u64* __restrict__ slab, uint32_t rows, uint32_t n, uint32_t tick, uint32_t channels,
                                           unsigned char* __restrict__ out) {
    constexpr int SUMW = stats_sum_words(D), WORDS = (int)stats_words(D);
    const int w = (int)blockIdx.x;                                      // < WORDS: the grid
    const bool sum = w < SUMW;
    u64 acc = 0ull;
    for (uint32_t r = threadIdx.x; r < rows; r += 64u) {
        const u64 x = slab[(size_t)r * WORDS + w];
        acc = sum ? acc + x : (x > acc ? x : acc);
    }
    const u64 total = sum ? (u64)wave_sum((long long)acc) : 0ull;
    const uint32_t key = sum ? 0u : wave_umax((uint32_t)acc);
    if (threadIdx.x != 0u) return;
    int off = 0;
    bool is_min = false;
#pragma unroll
    for (int i = 0; i < WORDS; ++i)
        if (i == w) { off = stats_word_offset(D, i); is_min = i >= SUMW && stats_key_is_min(D, i - SUMW); }
    if (sum) *(u64*)(out + off) = total;
    else *(float*)(out + off) = stats_unkey(is_min ? ~key : key);
    if (w == 0) {
        *(u64*)out = (u64)n;
        *(uint32_t*)(out + stats_attr_offset(D) - 4) = tick;
        *(uint32_t*)(out + stats_attr_offset(D) + 96) = channels;
        *(uint32_t*)(out + stats_attr_offset(D) + 100) = 0u;
    }
}

}  // namespace fsd
