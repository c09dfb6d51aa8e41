// kernels_sort.hip — the reference's bitonic network (sort.wgsl:27-51, schedule
// src/simulation.rs:323-347) on 8-byte (key<<32 | source index) pairs.
//
// The reference issues S(S+1)/2 full-array dispatches over 32-byte records.  The network is
// data-oblivious and compares keys only (strict `>`, so equal keys never swap), hence sorting
// pairs and gathering the payload afterwards yields the bit-identical arrangement.  Structure:
//   * k_bitonic_local<INIT,KEYGEN>: predict + key (compute.wgsl:8-42) fused into the tile load, then
//                                   stages 0..11 entirely inside a 4096-pair tile (registers + LDS);
//   * k_bitonic_strided<M,FLIP>:    up to M steps of a later stage whose partners lie in different
//                                   tiles, in registers (one HBM/MALL pass per M steps);
//   * k_bitonic_local<TAIL>:        the last 12 steps of a stage, inside a tile.
// Provable no-ops are skipped (per-tile dirty flags, ordered-chunk certificates): see the
// comments at k_bitonic_local and k_bitonic_strided.
// Elements at index >= n do not exist in the reference (`if index_high >= num_values return`,
// sort.wgsl:39-41); here they hold a sentinel pair that can never swap (its key is the u32
// maximum and the compare is strict), which is equivalent.
//
// This file is the host schedule: which kernels one sort call puts into the stream, in which order.  The kernels and
// their launch functions are in kernels_sort_tile.inc (inside a tile) and kernels_sort_global.inc (across tiles, the
// late-stage certificate and the stand-by kernel); fs_sort.h holds what the three share.  The schedule reaches the
// kernels through the launch functions of fs_sort.h only; the two kernel files are compiled as part of this
// translation unit all the same, see the end of the file.
#include "fs_kernels.h"
#include "fs_sort.h"

namespace fsd {

// Elements per thread of the tile kernels (2^3 or 2^4, fs_sort_tile.h), chosen per sort from the tile count (both forms
// are compiled): FS_SORT_GB in the environment pins one.
static int sort_gb(uint32_t tiles) {
    const SortKnobs& K = sort_knobs();
    if (K.gb == 3 || K.gb == 4) return K.gb;
    // few tiles cannot fill the chip: shorter per-thread chains win there.  Sort pass, ms, 8 / 16 elements per thread:
    // 1M (256 tiles) 0.066 / 0.078, 2M 0.094 / 0.098, 4M 0.142 / 0.136, 8M 0.253 / 0.250, 16M 0.445 / 0.435
    return tiles <= K.gb3_tiles ? 3 : 4;
}

// First stage handled by the shifted merge (0: never; the proof is at k_late_cert).  Default S - 6: windows of +-2^(S-7)
// elements, sixteen grid rows of the square dam-break scenes (a row holds 2 sqrt(n) particles).  Measured at 16M (S = 24),
// sort pass, ms:
//   steps 10-110: none 0.729, 16: 0.618, 17: 0.641, 18: 0.648, 19: 0.666;  steps 150-250 (dense floor, fuller rows):
//   none 0.802, 16 / 17: 0.82 (the certificate fails, per-stage plan + 3 idle launches), 18: 0.718, 19: 0.740.
static int sort_fuse_stage(uint32_t S, int request) {
    const int want = request >= 0 ? request : sort_knobs().fuse_stage;
    int s0 = want >= 0 ? want : (int)S - 6;
    if (want < 0 && s0 < SORT_LOG_T + 1) s0 = SORT_LOG_T + 1;
    if (s0 < SORT_LOG_T + 1 || s0 >= (int)S) return 0;          // H must be a whole number of tiles; something must be left
    return s0;
}

uint32_t sort_tile_count(uint32_t n) {
    uint32_t p2 = 1;
    while (p2 < n) p2 <<= 1;
    return (p2 + SORT_T - 1) / SORT_T + 1u + SORT_PW_COUNT;  // tiles of the padded array (sentinel tiles included) + the plan words
}
uint32_t sort_plan_word(uint32_t n) { return sort_tile_count(n) - SORT_PW_COUNT; }

// One stage >= SORT_LOG_T of the network on `pairs[0 .. n)`: its strided passes, then the tile tails.
static int launch_stage(hipStream_t st, u64* pairs, uint32_t n, uint32_t p2, uint32_t stage, uint32_t* dirty, int mmax,
                        int try_skip, const uint32_t* gate, uint32_t glo, uint32_t ghi) {
    const uint32_t tiles = (n + SORT_T - 1) / SORT_T;
    // steps whose block (2 << sh) exceeds the tile: sh = stage .. SORT_LOG_T, in passes of <= mmax steps
    const int gsteps = (int)(stage - SORT_LOG_T + 1);
    const int npass = (gsteps + mmax - 1) / mmax;
    uint32_t a = stage;
    for (int ps = 0; ps < npass; ++ps) {
        const int m = sort_pass_steps(gsteps, npass, ps);
        launch_sort_strided(st, pairs, n, a, m, ps == 0, p2, dirty, try_skip, gate, glo, ghi);
        a -= (uint32_t)m;
    }
    launch_sort_tails(st, pairs, n, dirty, sort_gb(tiles), gate, glo, ghi);
    return npass + 1;
}

int launch_bitonic_sort(hipStream_t st, u64* pairs, uint32_t n, uint32_t* dirty, const SortKeys* keys, const SortPlan* plan) {
    if (n <= 1) return 0;
    const SortKnobs& K = sort_knobs();
    uint32_t p2 = 1, S = 0;
    while (p2 < n) { p2 <<= 1; ++S; }
    const int gb = sort_gb((n + SORT_T - 1) / SORT_T);
    int launches = launch_sort_first(st, pairs, n, S < SORT_LOG_T ? S : SORT_LOG_T, dirty, keys, gb, K.packed);
    const uint32_t s0 = (uint32_t)sort_fuse_stage(S, plan ? plan->fuse_stage : -1);
    uint32_t* gate = dirty + sort_plan_word(n);           // the plan words; SORT_PW_VERDICT, the first, gates the launches
    static_assert(SORT_PW_VERDICT == 0, "the gate is the first plan word");
    for (uint32_t stage = SORT_LOG_T; stage < S; ++stage) {
        const int mmax = (int)stage >= K.late_stage ? K.mmax_late : K.mmax;
        const int ts = (K.skip_stage >= 0 && (int)stage >= K.skip_stage) ? 1 : 0;
        if (s0 && stage == s0) {
            // verdict, then the shifted merge (runs when the verdict is s0); stages s0 .. S-1 below run when it is FS_SORT_NO_PLAN
            const uint32_t H = 1u << (s0 - 1u);
            launch_sort_cert(st, pairs, n, p2, s0, gate, K.cert_block, plan ? plan->feedback : nullptr, plan ? plan->seq : 0u);
            ++launches;
            if (n > H) launches += launch_stage(st, pairs + H, n - H, p2, s0 - 1u, dirty + (H >> SORT_LOG_T), K.mmax_shifted, 1, gate, s0, s0);
            if (plan && plan->fallback == 1) {         // everything the certificate may still ask for, in one launch
                launch_sort_fallback(st, pairs, n, p2, S, s0, dirty, gate, K.fallback_grid, plan->inject_timeout != 0);
                return launches + 1;
            }
        }
        // a stage at or after the verdict's is already done: these launches then return at once (~5 us each)
        const bool gated = s0 && stage >= s0;
        if (stage == SORT_LOG_T && K.fused12) {        // (never gated: s0 > SORT_LOG_T)
            launch_sort_stage12(st, pairs, n, gb);
            ++launches;
            continue;
        }
        launches += launch_stage(st, pairs, n, p2, stage, dirty, mmax, ts, gated ? gate : nullptr, stage + 1u, FS_SORT_NO_PLAN);
    }
    return launches;
}

}  // namespace fsd

// One translation unit for the device code, on purpose.  k_late_fallback (kernels_sort_global.inc) and the tile tails
// k_bitonic_local<false, 0, 4> (kernels_sort_tile.inc) are the two users of lt_tail<4>, and what the optimiser makes of
// each depends on the other being in the same module: compiled apart, with not a character of device code changed,
// k_late_fallback comes out with 173 instead of 174 VGPRs and 660 of its 5786 lines different, the tails with 40 of 1303
// lines different (tools/isa_compare.py) — and the tails carry every stage >= 13 of a 16M sort.  Compiled here, all 28
// kernels are instruction for instruction what they were (profiles/sort_split_resource_usage.txt).  Making the two
// files sources of their own is dropping these two lines and listing them in build.py, once those two kernels have
// been measured in their other form.
// (Global before tile, and inside the files the launch functions in the order they stand: the kernels are laid out in
// the code object in the order their launches are first seen, and this order is the one every measurement was made with.)
#include "kernels_sort_global.inc"
#include "kernels_sort_tile.inc"
