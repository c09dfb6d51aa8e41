// engine_3d_count.hip — a particle count that changes at run time (include/fluidsim.h "3D particle count"; the
// handle: engine_3d.h, the device passes: kernels_count.hip): fs3_reserve grows every per-slot array, fs3_emit_* append at
// [n, n + m), fs3_remove_* compact.  The live count is always known to the host: the step's pass chain and its kernels are
// untouched, each step simply takes the n of its enqueue.  The 2D handle's counterpart: engine_count.hip; what the two share:
// engine_count.h.
#include <hip/hip_runtime.h>

#include "engine_3d.h"
#include "engine_count.h"

using namespace fsd;
namespace {
// The count becomes new_n (2 <= new_n <= cap, != n), the state arrays already hold it (or will, in stream order).  What every
// change shares: the queries, surface tension's forces and buoyancy's no longer belong to the state, and the sort's bookkeeping follows
// (sort_count_changed).
fs_status count_changed(fs_sim3* s, uint32_t new_n) {
    const fs_status health = sort_count_changed(s->stream, s->sortp, s->dirty, s->n, new_n);
    s->n = new_n;
    s->sample_stale = true;
    s->tension.valid = false;
    s->diffusion.valid = false;
    return health;
}

// The removal both forms end in: removal.flags (device, n bytes) and removal.sums are filled.  Blocking.
fs_status remove3(fs_sim3* s, uint32_t* removed) {
    const uint32_t n = s->n;
    uint32_t keep = 0;
    FS_TRY(removal_survivors(s->stream, s->removal, n, &s->sortp, s->dirty.p, &keep));
    if (keep == n) return FS_OK;                          // nothing matched: nothing changes, queries stay valid
    // out of place: positions and velocities into the spare arrays, pred (+ density) and keys into the AoS staging buffer
    // (48 B per slot: cap float4, then cap words) and back; ids and channels into tracking's other set
    Compact3 C{};
    C.pos = s->pos.p; C.vel = s->vel.p; C.pred = s->pred.p; C.key = s->key.p;
    C.pos_out = s->pos_s.p; C.vel_out = s->vel_s.p;
    C.pred_out = (float4*)s->aos.p; C.key_out = (uint32_t*)((float4*)s->aos.p + s->cap);
    compact_tracking(&C, s->trk, s->cap);
    launch3_remove_scatter(s->stream, n, s->removal.flags.p, s->removal.sums.p, C);
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpyAsync(s->pred.p, C.pred_out, (size_t)keep * sizeof(float4), hipMemcpyDeviceToDevice, s->stream));
    FS_HIP(hipMemcpyAsync(s->key.p, C.key_out, (size_t)keep * 4, hipMemcpyDeviceToDevice, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    std::swap(s->pos, s->pos_s);
    std::swap(s->vel, s->vel_s);
    if (s->trk.on()) s->trk.cur ^= 1;
    const fs_status r = count_changed(s, keep);
    FS_HIP(hipStreamSynchronize(s->stream));
    *removed = n - keep;
    return r;
}
}  // namespace

extern "C" {

uint32_t fs3_capacity(const fs_sim3* s) { return s ? s->cap : 0; }
uint32_t fs3_track_next_id(const fs_sim3* s) { return (s && s->trk.on()) ? s->trk.next_id : 0; }

fs_status fs3_reserve(fs_sim3* s, uint32_t capacity) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (capacity > MAX_SLOTS) return fail(FS_ERR_INVALID, "capacity > 2^28 (32-bit byte offsets)");
    if (capacity <= s->cap) return FS_OK;
    FS_HIP(hipSetDevice(s->device));
    const size_t cap = capacity, n = s->n;
    // everything new first: on failure the locals go and the handle is what it was
    DevArray<float4> pos, vel, pos_s, vel_s, pred, st, fb;
    DevArray<uint32_t> key, dirty;
    DevArray<u64> pairs, masks;
    DevArray<fs3_particle> aos;
    TrackingGrowth G;
    hipError_t e = hipSuccess;
    auto ok = [&e](hipError_t r) { e = r; return r == hipSuccess; };
    (void)(ok(pos.alloc(cap)) && ok(vel.alloc(cap)) && ok(pos_s.alloc(cap)) && ok(vel_s.alloc(cap)) && ok(pred.alloc(cap + FS_PRED_SLACK)) &&
           ok(key.alloc(cap)) && ok(pairs.alloc(cap)) && ok(dirty.alloc(sort_tile_count(capacity))) && ok(aos.alloc(cap)) &&
           ok(masks.alloc(s->masks.p ? 18 * cap : 0)) && ok(st.alloc(s->tension.st.p ? cap : 0)) && ok(fb.alloc(s->diffusion.fb.p ? cap : 0)) &&
           ok(G.alloc(s->trk, cap)));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FS_ERR_OOM, "reserve: device arrays");
    }
    // behind the steps in flight: the state, the last step's sorted arrays (the queries read them) and forces, the sort's words
    hipStream_t q = s->stream;
    if (e == hipSuccess) e = hipMemsetAsync(dirty.p, 0, dirty.n * 4, q);
    if (e == hipSuccess) e = carry(q, dirty, s->dirty, s->dirty.n);       // tile flags and plan words keep their places: they follow n
    if (e == hipSuccess) e = carry(q, pos, s->pos, n);
    if (e == hipSuccess) e = carry(q, vel, s->vel, n);
    if (e == hipSuccess) e = carry(q, pos_s, s->pos_s, n);
    if (e == hipSuccess) e = carry(q, vel_s, s->vel_s, n);
    if (e == hipSuccess) e = carry(q, pred, s->pred, n);
    if (e == hipSuccess) e = carry(q, key, s->key, n);
    if (e == hipSuccess) e = carry(q, st, s->tension.st, n);
    if (e == hipSuccess) e = carry(q, fb, s->diffusion.fb, n);
    if (e == hipSuccess) e = G.carry_from(q, s->trk, n, s->cap, cap);
    const hipError_t es = hipStreamSynchronize(q);                         // before anything is freed, whatever happened
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(FS_ERR_DEVICE, hipGetErrorString(e));
    s->pos = std::move(pos); s->vel = std::move(vel); s->pos_s = std::move(pos_s); s->vel_s = std::move(vel_s); s->pred = std::move(pred);
    s->key = std::move(key); s->pairs = std::move(pairs); s->dirty = std::move(dirty); s->aos = std::move(aos);
    if (masks.p) s->masks = std::move(masks);
    if (st.p) s->tension.st = std::move(st);
    if (fb.p) s->diffusion.fb = std::move(fb);
    G.commit(s->trk);
    s->removal.release();                                                  // sized by the capacity: the next removal allocates it again
    s->cap = capacity;
    return sort_health3(s);
}

fs_status fs3_emit_particles(fs_sim3* s, const fs3_particle* src, size_t n) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (n == 0) return FS_OK;
    if (!src) return fail(FS_ERR_INVALID, "null argument");
    if (n > (size_t)(s->cap - s->n)) return fail(FS_ERR_INVALID, "emit: count + n exceeds the capacity (fs3_reserve first)");
    FS_HIP(hipSetDevice(s->device));
    // as fs3_upload_particles stores them, at slot `count`: through the staging buffer, which has cap >= n slots
    Arrays3 A = s->arrays();
    A.pos += s->n; A.pred += s->n; A.vel += s->n; A.key += s->n;
    FS_HIP(hipMemcpyAsync(s->aos.p, src, n * sizeof(fs3_particle), hipMemcpyHostToDevice, s->stream));
    launch3_import(s->stream, (uint32_t)n, A);
    FS_HIP(hipGetLastError());
    s->trk.emitted(s->stream, s->n, (uint32_t)n, s->cap);
    FS_HIP(hipStreamSynchronize(s->stream));               // `src` belongs to the caller again
    return count_changed(s, s->n + (uint32_t)n);
}

fs_status fs3_emit_nozzle(fs_sim3* s, const fs3_nozzle* z) {
    static_assert(sizeof(fs3_nozzle) == 56, "fs3_nozzle is 56 bytes");
    if (!s || !z) return fail(FS_ERR_INVALID, "null argument");
    const uint64_t m = (uint64_t)z->nu * z->nv;
    if (z->nu == 0u || z->nv == 0u || m > MAX_SLOTS) return fail(FS_ERR_INVALID, "nozzle: nu * nv must be 1 .. 2^28");
    const fs_vec3 f[4] = {z->origin, z->u, z->v, z->velocity};
    for (const fs_vec3& a : f)
        if (!std::isfinite(a.x) || !std::isfinite(a.y) || !std::isfinite(a.z)) return fail(FS_ERR_INVALID, "nozzle: non-finite component");
    if (m > (uint64_t)(s->cap - s->n)) return fail(FS_ERR_INVALID, "emit: count + nu * nv exceeds the capacity (fs3_reserve first)");
    FS_HIP(hipSetDevice(s->device));
    Nozzle3 Z;
    Z.origin = make_float3(z->origin.x, z->origin.y, z->origin.z); Z.u = make_float3(z->u.x, z->u.y, z->u.z);
    Z.v = make_float3(z->v.x, z->v.y, z->v.z); Z.velocity = make_float3(z->velocity.x, z->velocity.y, z->velocity.z);
    Z.nu = z->nu; Z.nv = z->nv;
    launch3_emit_nozzle(s->stream, Z, s->n, s->arrays());
    FS_HIP(hipGetLastError());
    s->trk.emitted(s->stream, s->n, (uint32_t)m, s->cap);
    return count_changed(s, s->n + (uint32_t)m);
}

fs_status fs3_remove_in_box(fs_sim3* s, const fs_vec3* lo, const fs_vec3* hi, uint32_t* removed) {
    if (removed) *removed = 0;
    if (!s || !lo || !hi || !removed) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(s->removal.reserve(s->cap));
    launch3_remove_box(s->stream, s->n, s->pos.p, make_float3(lo->x, lo->y, lo->z), make_float3(hi->x, hi->y, hi->z), s->removal.flags.p,
                            s->removal.sums.p);
    return remove3(s, removed);
}

fs_status fs3_remove_flagged(fs_sim3* s, const uint8_t* flags, size_t n, uint32_t* removed) {
    if (removed) *removed = 0;
    if (!s || !flags || !removed) return fail(FS_ERR_INVALID, "null argument");
    if (n != s->n) return fail(FS_ERR_INVALID, "removal: n must equal the particle count");
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(s->removal.reserve(s->cap));
    FS_HIP(hipMemcpyAsync(s->removal.flags.p, flags, n, hipMemcpyHostToDevice, s->stream));
    launch_remove_count_flags(s->stream, s->n, s->removal.flags.p, s->removal.sums.p);
    return remove3(s, removed);
}

}  // extern "C"
