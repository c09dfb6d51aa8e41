// fs_sort.h — what the host schedule (kernels_sort.hip) and the kernel files of the bitonic sort (kernels_sort_tile.inc,
// kernels_sort_global.inc) share: the tile size, the plan words, the launch gate, the environment knobs and the launch
// functions the schedule calls.  The public entry points (launch_bitonic_sort, sort_tile_count, sort_plan_word) are
// declared in fs_kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "fs_kernels.h"

namespace fsd {

#define SORT_LOG_T 12
#define SORT_T (1u << SORT_LOG_T)
#define FS_TILE_WIDE 2u      // dirty[tile]: the packed first kernel left this tile to the 64-bit one (k_bitonic_local32)
#define FS_SORT_NO_PLAN 255u // verdict: the certificate failed, the per-stage plan (or the stand-by kernel) does stages s0 .. S-1

// The plan words: SORT_PW_COUNT u32 behind the tile flags, dirty[sort_plan_word(n) + word], zero at create.
// Fit class: the largest j <= 3 for which (C2), (C3) of k_late_cert still hold with windows of H / 2^j — how much room the
// moves of this step left; the host's choice of the next steps' stage reads it (sort_policy.h), never the result.
enum SortPlanWord : uint32_t {
    SORT_PW_VERDICT = 0,       // k_late_cert: the first stage the shifted merge replaces, or FS_SORT_NO_PLAN (the launch gate)
    SORT_PW_SHIFTED = 1,       // diagnostics: calls that took the shifted merge ...
    SORT_PW_PER_STAGE = 2,     // ... and calls whose certificate failed
    SORT_PW_BARRIER = 3,       // k_late_fallback: its grid barrier's counter (reset by the certificate)
    SORT_PW_TIMEOUTS = 4,      // ... and the barrier time-outs (sort_policy.h: the handle is dead from then on)
    SORT_PW_FIT_CLASS = 5,     // fit class of the last certificate
    SORT_PW_STANDBY_RUNS = 6,  // calls in which the stand-by kernel had work
    SORT_PW_WIDE_TILES = 7,    // tiles the packed first kernel flagged FS_TILE_WIDE (fs_sort_plan_info.wide_tiles)
    SORT_PW_CERT_BITS = 8,     // k_late_cert's grid: the workgroups' failure bits ...
    SORT_PW_CERT_TICKET = 9,   // ... and their ticket (the last to arrive publishes the verdict)
    SORT_PW_COUNT = 16
};

// Late-stage plans (see k_late_cert): `*gate` holds the certificate's verdict; a launch runs when it lies in [lo, hi].
__device__ __forceinline__ bool gate_closed(const uint32_t* gate, uint32_t lo, uint32_t hi) {
    if (!gate) return false;
    const uint32_t v = *gate;
    return v < lo || v > hi;
}

// A stage's `gsteps` global steps are split evenly over `npass` passes, the longer passes first: steps of pass `ps`.
__host__ __device__ __forceinline__ int sort_pass_steps(int gsteps, int npass, int ps) {
    return gsteps / npass + (ps < gsteps % npass ? 1 : 0);
}

// The environment knobs of the sort, read once per process (sort_knobs()).  Nothing else reads these names.
struct SortKnobs {
    // FS_SORT_GB: elements per thread of the tile kernels (2^3 or 2^4; both forms are compiled); anything else: chosen per
    // sort from the tile count, see sort_gb() in kernels_sort.hip for the measurements.
    int gb = env("FS_SORT_GB", 0);
    uint32_t gb3_tiles = (uint32_t)env("FS_SORT_GB3_TILES", 512);   // ... up to this many tiles: 8 elements per thread
    // FS_SORT_MMAX: steps per strided pass.  Measured over the bench window @16M: 2: 0.90 ms, 3: 0.74, 4: 0.706, 5: 0.718, 6: 0.79
    int mmax = clamp(env("FS_SORT_MMAX", 4), 1, 6);
    // Late stages (2^stage far beyond the distance a particle's key moves in one step) are almost entirely certified
    // no-ops: their cost is the launch count, so they take more steps per pass.
    int mmax_late = clamp(env("FS_SORT_MMAX_LATE", 4), 1, 6);
    int mmax_shifted = clamp(env("FS_SORT_MMAX_SHIFTED", 4), 1, 6);   // the shifted merge's stage
    int late_stage = env("FS_SORT_LATE_STAGE", 18);                 // first stage that takes mmax_late
    int skip_stage = env("FS_SORT_SKIP_STAGE", 12);   // first stage whose strided passes try the no-op certificate (<0: never)
    int fuse_stage = env("FS_SORT_FUSE_STAGE", -1);   // first stage of the shifted merge, see sort_fuse_stage() (< 0: default)
    // engines' steps (the pairs are built by the first kernel): the packed kernel first, then the 64-bit kernel for the tiles
    // it flagged FS_TILE_WIDE (an idle launch in a running simulation).  FS_SORT_PACKED=0: the 64-bit kernel alone, as in round 2.
    bool packed = env("FS_SORT_PACKED", 1) != 0;
    bool fused12 = env("FS_SORT_FUSED12", 1) != 0;    // stage 12 in one kernel (k_bitonic_stage12)
    // k_late_cert: one boundary per thread, 16-thread workgroups: the key reads' address translations spread over the chip
    uint32_t cert_block = (uint32_t)clamp(env("FS_SORT_CERT_BLOCK", 16), 1, 256);
    // k_late_fallback: one workgroup per CU at most: all of them resident whatever else the kernel shares the chip with.
    // 16M, 16 working calls in 110: 64: sort 1.08 ms avg, 128: 1.01, 256: 1.12
    // (The default asks HIP for the CU count of the device that is current at the process's first sort, not, as before,
    // at its first stand-by launch: the same on a machine of equal devices.)
    int fallback_grid = clamp(env("FS_SORT_FALLBACK_GRID", default_fallback_grid()), 1, 256);

  private:
    static int env(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }
    static int clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
    static int default_fallback_grid() {
        int dev = 0, cus = 64;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        return cus > 128 ? 128 : cus;
    }
};
inline const SortKnobs& sort_knobs() {
    static const SortKnobs k;
    return k;
}

// ---- the launch functions of the two kernel files: all the schedule sees of them.  gb: 3 or 4 (LT<GB>, fs_sort_tile.h).
// kernels_sort_tile.inc
// Stages 0 .. min(S, 12) - 1 inside every tile (`keys`: null or what builds the pairs, see SortKeys); leaves every tile
// sorted and its flag cleared.  Returns the launches issued (the packed form is two: k_bitonic_local32, then the 64-bit
// kernel for the tiles it flagged).
int launch_sort_first(hipStream_t st, u64* pairs, uint32_t n, uint32_t init_stages, uint32_t* dirty, const SortKeys* keys,
                      int gb, bool packed);
// The last 12 steps of a stage >= 12, on the tiles flagged dirty.
void launch_sort_tails(hipStream_t st, u64* pairs, uint32_t n, uint32_t* dirty, int gb, const uint32_t* gate, uint32_t glo,
                       uint32_t ghi);
void launch_sort_stage12(hipStream_t st, u64* pairs, uint32_t n, int gb);
// kernels_sort_global.inc
// m (1 .. 6) global steps of a stage from bit `a` down, the first of them the stage's mirror step when `flip`.
void launch_sort_strided(hipStream_t st, u64* pairs, uint32_t n, uint32_t a, int m, bool flip, uint32_t p2, uint32_t* dirty,
                         int try_skip, const uint32_t* gate, uint32_t glo, uint32_t ghi);
void launch_sort_cert(hipStream_t st, const u64* pairs, uint32_t n, uint32_t p2, uint32_t s0, uint32_t* plan_words,
                      uint32_t cert_block, uint32_t* feedback, uint32_t seq);
void launch_sort_fallback(hipStream_t st, u64* pairs, uint32_t n, uint32_t p2, uint32_t S, uint32_t s0, uint32_t* dirty,
                          uint32_t* plan_words, int grid, bool inject_timeout);

}  // namespace fsd
