// engine_selftest.hip — the self-tests of the C ABI (the constant-division proof, the sort and its plan policy on caller-supplied
// input) and the read-outs of what a handle proved and planned.  None of it is on a step's path.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "engine.h"
#include "fs_sort.h"

using namespace fsd;

extern "C" {

/* Exhaustive proof used by the force pass: number of f32 x with lo <= |x| <= hi for which the 3-op
 * constant division (x*y, fma, fma with the given reciprocal y) differs from the IEEE x / c.  Blocking. */
fs_status fs_selftest_constdiv(int device, float c, float y, float lo, float hi, uint32_t* mismatches) {
    if (!mismatches || !(lo > 0.0f) || !(hi >= lo) || !std::isfinite(hi)) return fail(FS_ERR_INVALID, "bad argument");
    FS_TRY(use_device(device, FS_ERR_DEVICE));
    DevArray<uint32_t> dm;
    FS_HIP(dm.alloc(1));
    FS_HIP(hipMemset(dm.p, 0, sizeof(uint32_t)));
    fsd::launch_verify_constdiv(nullptr, c, y, lo, hi, dm.p);
    hipError_t e = hipMemcpy(mismatches, dm.p, sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(FS_ERR_DEVICE, hipGetErrorString(e));
    return FS_OK;
}

/* The sort on caller-supplied pairs (tests of the late-stage plans on adversarial inputs).  Blocking. */
fs_status fs_selftest_sort(int device, uint64_t* pairs, uint32_t n, int fuse_stage, uint32_t plan[2]) {
    if (!pairs || n == 0 || n > (1u << 28)) return fail(FS_ERR_INVALID, "bad argument");
    FS_TRY(use_device(device, FS_ERR_DEVICE));
    DevArray<u64> dp;
    DevArray<uint32_t> dd;      // the tile flags and, behind them, the plan words
    FS_HIP(dp.alloc(n));
    hipError_t e = dd.alloc(fsd::sort_tile_count(n));
    if (e == hipSuccess) e = hipMemset(dd.p, 0, dd.n * 4);
    if (e == hipSuccess) e = hipMemcpy(dp.p, pairs, (size_t)n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        fsd::SortPlan sp;
        sp.fuse_stage = fuse_stage < 0 ? -1 : (fuse_stage & 0xFF);
        sp.fallback = fuse_stage >= 0 && (fuse_stage & 0x100) ? 1 : 0;
        fsd::launch_bitonic_sort(nullptr, dp.p, n, dd.p, nullptr, &sp);
        e = hipMemcpy(pairs, dp.p, (size_t)n * 8, hipMemcpyDeviceToHost);
    }
    static_assert(fsd::SORT_PW_PER_STAGE == fsd::SORT_PW_SHIFTED + 1, "plan[2] is read in one copy");
    if (e == hipSuccess && plan) e = hipMemcpy(plan, dd.p + fsd::sort_plan_word(n) + fsd::SORT_PW_SHIFTED, 8, hipMemcpyDeviceToHost);   // ... and SORT_PW_PER_STAGE
    uint32_t timeouts = 0;
    if (e == hipSuccess) e = hipMemcpy(&timeouts, dd.p + fsd::sort_plan_word(n) + fsd::SORT_PW_TIMEOUTS, 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(FS_ERR_DEVICE, hipGetErrorString(e));
    if (timeouts) return fail(FS_ERR_DEVICE, "sort fallback: grid barrier timed out");
    return FS_OK;
}

/* The plan policy replayed against a model of the flow (include/fluidsim.h); host only. */
fs_status fs_selftest_sort_policy(uint32_t S, int start_back, uint32_t lag, const uint32_t* required, size_t steps,
                                  uint32_t* stage_out, uint32_t* single_out) {
    if (!required || !stage_out || !single_out || S < 15 || S > 28) return fail(FS_ERR_INVALID, "bad argument");
    fsd::SortPolicy p;
    p.start_back = start_back;
    std::vector<uint32_t> used(steps);
    for (size_t i = 0; i < steps; ++i) {
        if (i >= lag && i - lag < steps) {             // the report of step i - lag arrives before step i is planned
            const size_t j = i - lag;
            const int st = (int)used[j];
            const bool passed = st >= (int)required[j];
            const int cls = passed ? (st - (int)required[j] > 3 ? 3 : st - (int)required[j]) : 0;
            p.observe((uint32_t)j + 1u, st, passed, cls, S);
        }
        used[i] = (uint32_t)(p.stage ? p.stage : p.first_stage(S));
        p.seq = (uint32_t)i + 1u;                      // what plan() does: this step's sequence number
        stage_out[i] = used[i];
        single_out[i] = p.single_standby() ? 1u : 0u;
    }
    return FS_OK;
}

fs_status fs_sort_plan_read(fs_sim* s, fs_sort_plan_info* out) {
    if (!s || !out) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipSetDevice(s->device));
    FS_HIP(hipStreamSynchronize(s->stream));
    uint32_t w[fsd::SORT_PW_COUNT] = {};
    const uint32_t count = s->slab ? s->capacity : s->n;
    if (count > 1) FS_HIP(hipMemcpy(w, s->sort_dirty.p + fsd::sort_plan_word(count), sizeof w, hipMemcpyDeviceToHost));
    out->shifted = w[fsd::SORT_PW_SHIFTED]; out->per_stage = w[fsd::SORT_PW_PER_STAGE]; out->standby_runs = w[fsd::SORT_PW_STANDBY_RUNS];
    out->timeouts = w[fsd::SORT_PW_TIMEOUTS]; out->wide_tiles = w[fsd::SORT_PW_WIDE_TILES];
    out->stage = (uint32_t)s->sortp.stage;
    out->standby_single = (s->sortp.force_single || (s->sortp.stage && s->sortp.trusted >= 2)) ? 1u : 0u;
    return FS_OK;
}

/* Did the create-time proofs succeed for this handle's constants (2h^3, h^2)?  Bits 0 / 1. */
int fs_constdiv_status(const fs_sim* s) {
    return s ? (s->div_2h3.ok ? 1 : 0) | (s->div_h2.ok ? 2 : 0) | (s->rcp_ok ? 4 : 0) | (s->sqrt_ok ? 8 : 0) | (s->div_h.ok ? 16 : 0) : 0;
}

}  // extern "C"
