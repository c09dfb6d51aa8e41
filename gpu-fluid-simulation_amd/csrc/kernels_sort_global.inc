// kernels_sort_global.inc — compiled only as part of kernels_sort.hip (see its last lines); include it nowhere else.
// The kernels of the bitonic sort that work across tiles, and their launch functions for the
// schedule (kernels_sort.hip):
//   * k_bitonic_strided<M,FLIP>: up to M steps of a stage >= 12 whose partners lie in different tiles, in registers (one
//                                HBM/MALL pass per M steps), behind an exact no-op certificate;
//   * k_late_cert:               the certificate of the late stages' shifted merge;
//   * k_late_fallback:           the per-stage plan of the late stages in one persistent launch (strided passes in batch
//                                form, tile tails from fs_sort_tile.h, a grid barrier between them).
#include "fs_device.h"
#include "fs_kernels.h"
#include "fs_sort.h"
#include "fs_sort_tile.h"

namespace fsd {

// M consecutive global steps of one stage in ONE pass, register-blocked: a thread owns the
// 2^M elements whose indices differ only in bits [a-M+1, a] (a = stage - first step), loads
// them (each load is a coalesced 512-B wave segment: consecutive lanes = consecutive
// columns), runs the M compare-exchange steps in VGPRs and stores them back.  No LDS, no
// barriers; HBM/MALL traffic per M steps = one read + one write of the pair array.
//
// FLIP: the first step of a stage compares x with its mirror x ^ (2^(a+1)-1)
// (sort.wgsl:32-36, `group_height - 2*h`).  In "virtual" indices v (upper-half rows read
// from p = v ^ (2^a - 1)) the mirror step is a plain distance-2^a step; the later steps of
// the pass act on upper-half rows in reversed physical order, so the compare is reversed
// there.  Indices >= n hold a never-moving sentinel (see file header).
//
// Exact skipping (try_skip): a workgroup covers 256 consecutive columns of its 2^M rows; each
// row's 256-element chunk lies in one tile.  If all those tiles are clean (sorted) a chunk's
// keys are bounded by its first and last element, and if the chunks are ordered
// last(chunk) <= first(next chunk) in PHYSICAL index order then every compare-exchange of
// the pass has key[lower index] <= key[higher index]: no swap can happen and the workgroup
// returns after reading 2 elements per row instead of the whole 2^M x 256 block.
// First / last key of row l (PHYSICAL order) of the 256-column chunk `chunk`, for the no-op certificate: a dirty
// row can never certify (its "range" is everything).
template <int M, bool FLIP>
__device__ __forceinline__ void strided_cert_row(const u64* __restrict__ pairs, uint32_t n, uint32_t a,
                                                 const uint32_t* __restrict__ dirty, uint32_t chunk, uint32_t l,
                                                 uint32_t* first, uint32_t* last) {
    constexpr int R = 1 << M;
    const uint32_t low = a - (uint32_t)M + 1u;
    const uint32_t mirror = (1u << a) - 1u;
    // row l in PHYSICAL order: lower half as is; with FLIP the upper half is mirrored, so its
    // rows appear in reverse order and each chunk is read back to front
    const bool upper = FLIP && (l >> (M - 1));
    const uint32_t rv = upper ? (uint32_t)(R - 1) - (l - (uint32_t)(R / 2)) : l;   // virtual row
    const uint32_t g0 = chunk * 256u, g1 = g0 + 255u;
    const uint32_t v0 = (((g0 >> low) << (a + 1u)) | (g0 & ((1u << low) - 1u))) | (rv << low);
    const uint32_t v1 = (((g1 >> low) << (a + 1u)) | (g1 & ((1u << low) - 1u))) | (rv << low);
    const uint32_t pf = upper ? (v1 ^ mirror) : v0;      // physically first / last element of the chunk
    const uint32_t pl = upper ? (v0 ^ mirror) : v1;
    const bool clean = pf >= n || dirty[pf >> SORT_LOG_T] == 0;   // past the end: sentinels, in order by definition
    const uint32_t kf = pf < n ? (uint32_t)(pairs[pf] >> 32) : 0xFFFFFFFFu;
    const uint32_t kl = pl < n ? (uint32_t)(pairs[pl] >> 32) : 0xFFFFFFFFu;
    *first = clean ? kf : 0u;
    *last = clean ? kl : 0xFFFFFFFFu;
}

template <int M, bool FLIP>
__device__ __forceinline__ void strided_body(u64* __restrict__ pairs, uint32_t n, uint32_t a, uint32_t num_threads,
                                             uint32_t* __restrict__ dirty, uint32_t g);

template <int M, bool FLIP>
__global__ __launch_bounds__(256) void k_bitonic_strided(u64* __restrict__ pairs, uint32_t n, uint32_t a,
                                                         uint32_t num_threads, uint32_t* __restrict__ dirty,
                                                         int try_skip, const uint32_t* __restrict__ gate,
                                                         uint32_t gate_lo, uint32_t gate_hi) {
    if (gate_closed(gate, gate_lo, gate_hi)) return;   // uniform: this launch belongs to the other late-stage plan
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    constexpr int R = 1 << M;
    if (try_skip) {                                    // uniform branch (kernel argument)
        __shared__ uint32_t s_first[R], s_last[R];
        __shared__ int s_skip;
        const uint32_t l = threadIdx.x;
        if (l < (uint32_t)R) strided_cert_row<M, FLIP>(pairs, n, a, dirty, blockIdx.x, l, &s_first[l], &s_last[l]);
        __syncthreads();
        if (l == 0) {
            int ok = 1;
#pragma unroll
            for (int r = 0; r < R; ++r) ok &= (s_first[r] <= s_last[r]);
#pragma unroll
            for (int r = 0; r + 1 < R; ++r) ok &= (s_last[r] <= s_first[r + 1]);
            s_skip = ok;
        }
        __syncthreads();
        if (s_skip) return;
    }
    strided_body<M, FLIP>(pairs, n, a, num_threads, dirty, g);
}

template <int M, bool FLIP>
__device__ __forceinline__ void strided_body(u64* __restrict__ pairs, uint32_t n, uint32_t a, uint32_t num_threads,
                                             uint32_t* __restrict__ dirty, uint32_t g) {
    constexpr int R = 1 << M;
    const uint32_t low = a - (uint32_t)M + 1u;
    const uint32_t mirror = (1u << a) - 1u;
    if (g >= num_threads) return;
    const uint32_t vbase = ((g >> low) << (a + 1u)) | (g & ((1u << low) - 1u));
    u64 x[R];
    u64 changed = 0;   // bit r set when x[r] took part in a swap: untouched elements are not stored
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t v = vbase | ((uint32_t)r << low);
        const uint32_t p = (FLIP && (r >> (M - 1))) ? (v ^ mirror) : v;
        x[r] = p < n ? pairs[p] : ~0ull;
    }
#pragma unroll
    for (int b = M - 1; b >= 0; --b) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (r & (1 << b)) continue;
            const int r1 = r | (1 << b);
            const bool rev = FLIP && b < M - 1 && (r >> (M - 1));   // upper half after the mirror step
            const uint32_t klo = (uint32_t)((rev ? x[r1] : x[r]) >> 32);
            const uint32_t khi = (uint32_t)((rev ? x[r] : x[r1]) >> 32);
            if (klo > khi) {
                const u64 t = x[r]; x[r] = x[r1]; x[r1] = t;
                changed |= (1ull << r) | (1ull << r1);
            }
        }
    }
    if (changed == 0) return;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t v = vbase | ((uint32_t)r << low);
        const uint32_t p = (FLIP && (r >> (M - 1))) ? (v ^ mirror) : v;
        if ((changed >> r) & 1ull) {                 // a sentinel (p >= n) never swaps, so p < n here
            pairs[p] = x[r];
            dirty[p >> SORT_LOG_T] = 1u;              // this tile's tail must run
        }
    }
}

// The same pass in batch form, for the persistent stand-by kernel (k_late_fallback): a workgroup checks the
// certificates of K consecutive chunks in one round of loads (K * 2^M lanes, one row each), then runs the body on the
// chunks that failed.  Exact for any input (a chunk's body touches its own elements only).  As launches of their own
// the batch form and a tile-walking tail were measured slower than the plain kernels (profiles/r02_d_rejected.md).
template <int M>
struct StridedBatch { static constexpr int R = 1 << M; static constexpr int K = (256 / R) < 8 ? (256 / R) : 8; };

// One batch: the certificates of chunks c0 .. c0+K-1 in one round of loads, then the bodies of the chunks that failed.
// Ends with a barrier (the shared words are reusable on return).
template <int M, bool FLIP>
__device__ __forceinline__ void strided_batch(u64* pairs, uint32_t n, uint32_t a, uint32_t num_threads, uint32_t* dirty,
                                              uint32_t c0, uint32_t* s_first, uint32_t* s_last, uint32_t* s_active) {
    constexpr int R = StridedBatch<M>::R, K = StridedBatch<M>::K;
    const uint32_t nchunks = num_threads >> 8;          // whole 256-column chunks (launcher: num_threads >= 256, a power of two)
    const uint32_t l = threadIdx.x;
    if (l == 0) *s_active = 0;
    if (l < (uint32_t)(K * R) && c0 + l / (uint32_t)R < nchunks)
        strided_cert_row<M, FLIP>(pairs, n, a, dirty, c0 + l / (uint32_t)R, l % (uint32_t)R, &s_first[l], &s_last[l]);
    __syncthreads();
    if (l < (uint32_t)K && c0 + l < nchunks) {
        int ok = 1;
#pragma unroll
        for (int r = 0; r < R; ++r) ok &= (s_first[l * R + r] <= s_last[l * R + r]);
#pragma unroll
        for (int r = 0; r + 1 < R; ++r) ok &= (s_last[l * R + r] <= s_first[l * R + r + 1]);
        if (!ok) atomicOr(s_active, 1u << l);
    }
    __syncthreads();
    uint32_t act = *s_active;                           // uniform
    while (act) {
        const uint32_t k = (uint32_t)__builtin_ctz(act);
        act &= act - 1u;
        strided_body<M, FLIP>(pairs, n, a, num_threads, dirty, (c0 + k) * 256u + l);
    }
    __syncthreads();
}

// ---------------------------------------------------------------- late stages in one shifted merge
// After stage S0-1 the array is a sequence of sorted blocks of 2^S0 = 2H elements.  Between two consecutive steps
// of the simulation a particle's key moves by a few grid rows at most, so what the remaining stages S0 .. S-1 still
// have to do is confined to a neighbourhood of the block boundaries m = b 2^S0.  If, for every boundary,
//     (C2) key[m - H - 1] <= key[m]          (the part of the left block outside the window is below the right block)
//     (C3) key[m + H]     >= key[m - 1]      (the part of the right block outside the window is above the left block)
//     (C4) key[m - 1]     <= key[m + 2H]     (the left block is below the block after the next boundary)
// then, with the windows W_b = [m - H, m + H):
//   * the elements outside all windows are in non-decreasing order over the whole array and bound every window
//     from below / above; any two windows are ordered as sets (max W_b <= min W_b+1).  By induction over the
//     network's compare-exchanges no pair with an end outside a window, or with ends in two windows, ever swaps
//     (key[lower index] <= key[higher index] holds for it; the compare is strict, ties never swap);
//   * the pairs of stages >= S0 with BOTH ends in W_b are: the mirror pairs (m-1-i, m+i) of the one stage whose
//     block centre m is (m = odd * 2^stage), and the plain steps of distance <= H/2 inside the two halves (an aligned
//     pair of distance >= H straddles no window: m is a multiple of 2H).  The halves are sorted, so the plain
//     steps are no-ops before that stage; its mirror + plain steps are a bitonic merge of the halves; afterwards the
//     window is sorted and later plain steps are no-ops again.
// Hence stages S0 .. S-1 together equal ONE merge of every window — which is stage S0-1 of the same network run on
// the array shifted by H elements (tile aligned, H >= 4096): the kernels above, a pointer offset, 2-3 launches
// instead of 3-4 per remaining stage.  k_late_cert evaluates (C2)-(C4) on the device and publishes the verdict;
// the launches of both plans are in the stream and each returns at once unless the verdict names its plan, so the
// result is the network's in every case (uploads, fast flows: the conditions fail and the per-stage plan runs).
// Round 4: a grid of small workgroups instead of one of 256 threads.  The kernel's time was never its arithmetic: at 16 M
// particles it reads 512 x 11 keys 256 KB apart — every one a TLB miss, all of them queued on ONE compute unit's address
// translation (14.6 us, profiles/r03_window_5_25_kernels.txt).  Spread over the chip the misses are taken in parallel; the
// workgroups OR their failure bits into SORT_PW_CERT_BITS, and the last one to arrive (ticket SORT_PW_CERT_TICKET) publishes
// the verdict.  `plan`: the plan words (fs_sort.h SortPlanWord).
// feedback (optional, host-visible; sort_policy.h): [1] stage, [2] verdict, [3] fit class, [4] time-outs, then [0] = seq.
__global__ __launch_bounds__(256) void k_late_cert(const u64* __restrict__ pairs, uint32_t n, uint32_t p2, uint32_t s0,
                                                    uint32_t* __restrict__ plan, uint32_t* __restrict__ feedback,
                                                    uint32_t seq) {
    const uint32_t H = 1u << (s0 - 1u), nb = p2 >> s0;
    uint32_t bad = 0;                    // bit 0: (C2)-(C4) fail; bits 1..3: (C2), (C3) fail with windows of H/2, H/4, H/8
    // Eleven keys per boundary, all loaded before any is compared (clamped index, sentinel selected afterwards).
    for (uint32_t b = 1u + blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += gridDim.x * blockDim.x) {
        const uint32_t m = b << s0;
        const uint32_t idx[11] = {m - 1u, m, m - H - 1u, m + H, m + 2u * H, m - (H >> 1) - 1u, m + (H >> 1),
                                  m - (H >> 2) - 1u, m + (H >> 2), m - (H >> 3) - 1u, m + (H >> 3)};
        uint32_t k[11];
#pragma unroll
        for (int j = 0; j < 11; ++j) k[j] = (uint32_t)(pairs[idx[j] < n ? idx[j] : n - 1u] >> 32);
#pragma unroll
        for (int j = 0; j < 11; ++j) k[j] = idx[j] < n ? k[j] : 0xFFFFFFFFu;      // m + 2H == p2 reads as the sentinel
        const uint32_t left_max = k[0], right_min = k[1];
        if (!(k[2] <= right_min && k[3] >= left_max && left_max <= k[4])) bad |= 1u;
        if (!(k[5] <= right_min && k[6] >= left_max)) bad |= 2u;
        if (!(k[7] <= right_min && k[8] >= left_max)) bad |= 4u;
        if (!(k[9] <= right_min && k[10] >= left_max)) bad |= 8u;
    }
    __shared__ uint32_t s_bad;
    if (threadIdx.x == 0) s_bad = 0u;
    __syncthreads();
    if (bad) atomicOr(&s_bad, bad);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_bad) atomicOr(&plan[SORT_PW_CERT_BITS], s_bad);
        __threadfence();                               // the bits before the ticket
        if (atomicAdd(&plan[SORT_PW_CERT_TICKET], 1u) == gridDim.x - 1u) {
            __threadfence();
            const uint32_t bits = atomicExch(&plan[SORT_PW_CERT_BITS], 0u);              // all workgroups' bits; both words ready for the next call
            plan[SORT_PW_CERT_TICKET] = 0u;
            const bool all = (bits & 1u) == 0u;
            const uint32_t verdict = all ? s0 : FS_SORT_NO_PLAN;         // the first stage the shifted merge replaces, or none
            const uint32_t cls = !all ? 0u : !(bits & 8u) ? 3u : !(bits & 4u) ? 2u : !(bits & 2u) ? 1u : 0u;
            plan[SORT_PW_VERDICT] = verdict;
            atomicAdd(&plan[all ? SORT_PW_SHIFTED : SORT_PW_PER_STAGE], 1u);   // diagnostics: calls that took the shifted / the per-stage plan
            plan[SORT_PW_BARRIER] = 0;                  // the fallback kernel's barrier counter
            plan[SORT_PW_FIT_CLASS] = cls;
            if (feedback) {
                feedback[1] = s0; feedback[2] = verdict; feedback[3] = cls; feedback[4] = plan[SORT_PW_TIMEOUTS];
                __threadfence_system();
                feedback[0] = seq;
            }
        }
    }
}

// All workgroups of the grid have arrived `target / gridDim.x` times.  Release / acquire at agent scope around the
// counter make the passes' plain stores visible across workgroups (other XCDs' L2 included).  The spin is bounded:
// should the workgroups not all be resident (they are: the grid is far smaller than the chip) the kernel still ends,
// and the time-out is counted where the host reads it.
__device__ __forceinline__ void fallback_barrier(uint32_t* plan, uint32_t target) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(&plan[SORT_PW_BARRIER], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t spins = 0;
        while (__hip_atomic_load(&plan[SORT_PW_BARRIER], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(4);
            if (++spins > (1u << 22)) { atomicAdd(&plan[SORT_PW_TIMEOUTS], 1u); break; }
        }
    }
    __syncthreads();
}

template <int M>
__device__ __forceinline__ void fallback_pass(bool flip, u64* pairs, uint32_t n, uint32_t a, uint32_t p2, uint32_t* dirty,
                                              uint32_t* s_first, uint32_t* s_last, uint32_t* s_active) {
    const uint32_t threads = p2 >> M, nbatch = ((threads >> 8) + StridedBatch<M>::K - 1) / StridedBatch<M>::K;
    for (uint32_t b = blockIdx.x; b < nbatch; b += gridDim.x) {
        if (flip) strided_batch<M, true>(pairs, n, a, threads, dirty, b * StridedBatch<M>::K, s_first, s_last, s_active);
        else strided_batch<M, false>(pairs, n, a, threads, dirty, b * StridedBatch<M>::K, s_first, s_last, s_active);
    }
}

// The per-stage plan for stages s0 .. S-1 in ONE launch, for the steps whose certificate fails although the host
// expected it to hold (and therefore did not put the per-stage launches into the stream): a small persistent grid
// walks the passes in order with a grid barrier between them.  Rare (the host follows the fit class with a margin,
// sort_policy.h), correct for any input, several times slower than the per-stage launches when it has real work
// (16M: ~3.5 ms against 0.25 ms of per-stage launches: every barrier is an L2 write-back and invalidate).
__global__ __launch_bounds__(256) void k_late_fallback(u64* pairs, uint32_t n, uint32_t p2, uint32_t S, uint32_t s0,
                                                       uint32_t* dirty, uint32_t* plan, uint32_t inject_timeout) {
    if (plan[SORT_PW_VERDICT] != FS_SORT_NO_PLAN) return;   // uniform over the grid: the shifted merge did the work
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        atomicAdd(&plan[SORT_PW_STANDBY_RUNS], 1u);    // diagnostics: calls this kernel had to work in
        // tests only: report a time-out that did not happen (the barriers still hold, the sort stays correct), so that
        // the host's reaction — fs_step fails with FS_ERR_DEVICE from then on — has a test (tests/test_sort_gpu.py)
        if (inject_timeout) atomicAdd(&plan[SORT_PW_TIMEOUTS], 1u);
    }
    __shared__ u64 s[LT<4>::LDS];                       // 256 threads: the 16-element form of the tile code
    __shared__ uint32_t s_first[256], s_last[256];
    __shared__ uint32_t s_active;
    const uint32_t tiles = (n + SORT_T - 1) / SORT_T, t = threadIdx.x;
    uint32_t phase = 0;
    for (uint32_t stage = s0; stage < S; ++stage) {
        const int gsteps = (int)(stage - SORT_LOG_T + 1);
        const int npass = (gsteps + 3) / 4;
        uint32_t a = stage;
        for (int ps = 0; ps < npass; ++ps) {
            const int m = sort_pass_steps(gsteps, npass, ps);
            switch (m) {
                case 1: fallback_pass<1>(ps == 0, pairs, n, a, p2, dirty, s_first, s_last, &s_active); break;
                case 2: fallback_pass<2>(ps == 0, pairs, n, a, p2, dirty, s_first, s_last, &s_active); break;
                case 3: fallback_pass<3>(ps == 0, pairs, n, a, p2, dirty, s_first, s_last, &s_active); break;
                default: fallback_pass<4>(ps == 0, pairs, n, a, p2, dirty, s_first, s_last, &s_active); break;
            }
            a -= (uint32_t)m;
            fallback_barrier(plan, ++phase * gridDim.x);
        }
        for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
            if (dirty[tile] == 0) continue;            // uniform
            const uint32_t base = tile * SORT_T;
            u64 x[LT<4>::E];
            lt_tail<4>(pairs, n, base, s, x, t);
            lt_store<4>(pairs, s, x, base, t, n);
            if (t == 0) dirty[tile] = 0;
            __syncthreads();                           // the LDS stage is reused
        }
        fallback_barrier(plan, ++phase * gridDim.x);
    }
}

// ---- launch functions ------------------------------------------------------------------------------------------------
template <int M>
static void launch_strided(hipStream_t st, u64* pairs, uint32_t n, uint32_t a, bool flip, uint32_t p2,
                           uint32_t* dirty, int try_skip, const uint32_t* gate, uint32_t glo, uint32_t ghi) {
    const uint32_t threads = p2 >> M;
    const dim3 grid((threads + 255u) / 256u), block(256);
    if (threads < 256u) try_skip = 0;                  // the certificate assumes full 256-column workgroups
    if (flip) hipLaunchKernelGGL((k_bitonic_strided<M, true>), grid, block, 0, st, pairs, n, a, threads, dirty, try_skip, gate, glo, ghi);
    else hipLaunchKernelGGL((k_bitonic_strided<M, false>), grid, block, 0, st, pairs, n, a, threads, dirty, try_skip, gate, glo, ghi);
}

void launch_sort_strided(hipStream_t st, u64* pairs, uint32_t n, uint32_t a, int m, bool flip, uint32_t p2, uint32_t* dirty,
                         int try_skip, const uint32_t* gate, uint32_t glo, uint32_t ghi) {
    switch (m) {
        case 1: launch_strided<1>(st, pairs, n, a, flip, p2, dirty, try_skip, gate, glo, ghi); break;
        case 2: launch_strided<2>(st, pairs, n, a, flip, p2, dirty, try_skip, gate, glo, ghi); break;
        case 3: launch_strided<3>(st, pairs, n, a, flip, p2, dirty, try_skip, gate, glo, ghi); break;
        case 4: launch_strided<4>(st, pairs, n, a, flip, p2, dirty, try_skip, gate, glo, ghi); break;
        case 5: launch_strided<5>(st, pairs, n, a, flip, p2, dirty, try_skip, gate, glo, ghi); break;
        default: launch_strided<6>(st, pairs, n, a, flip, p2, dirty, try_skip, gate, glo, ghi); break;
    }
}

void launch_sort_cert(hipStream_t st, const u64* pairs, uint32_t n, uint32_t p2, uint32_t s0, uint32_t* plan_words,
                      uint32_t cert_block, uint32_t* feedback, uint32_t seq) {
    const uint32_t cert_nb = p2 >> s0;                 // one boundary per thread
    uint32_t cert_grid = (cert_nb + cert_block - 1u) / cert_block;
    if (cert_grid > 256u) cert_grid = 256u;
    if (cert_grid < 1u) cert_grid = 1u;
    hipLaunchKernelGGL(k_late_cert, dim3(cert_grid), dim3(cert_block), 0, st, pairs, n, p2, s0, plan_words, feedback, seq);
}

void launch_sort_fallback(hipStream_t st, u64* pairs, uint32_t n, uint32_t p2, uint32_t S, uint32_t s0, uint32_t* dirty,
                          uint32_t* plan_words, int grid, bool inject_timeout) {
    hipLaunchKernelGGL(k_late_fallback, dim3(grid), dim3(256), 0, st, pairs, n, p2, S, s0, dirty, plan_words,
                       inject_timeout ? 1u : 0u);
}

}  // namespace fsd
