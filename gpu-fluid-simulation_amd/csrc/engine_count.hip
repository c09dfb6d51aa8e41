// engine_count.hip — a particle count that changes at run time on the 2D handle (include/fluidsim.h "2D particle count",
// DESIGN.md §22; the handle: engine.h, the device passes: kernels_count.hip): fs_reserve grows every per-slot array, fs_emit_*
// append at [n, n + m), fs_remove_* compact.  The live count is always known to the host: the step's pass chain and its kernels
// are untouched, each step simply takes the n of its enqueue.  The 3D handle's counterpart: engine_3d_count.hip; what the two
// share: engine_count.h.
#include <hip/hip_runtime.h>

#include <cmath>

#include "engine_count.h"

using namespace fsd;
namespace {
const char* const SLAB = "slab handle: its particle count belongs to the exchange";

bool bitonic(const fs_sim* s) { return s->opts.sort_mode == FS_SORT_BITONIC; }

// State that is not at home: after a step the keys are the high words of `pairs` and, in strict / ulp mode,
// the densities are rho2.x.  Before a record is appended (its grid and density would be lost at the next read-out) or the
// state is compacted (stale `key` / `rho` would move), both go back to `key` / `rho`, as fs_upload_particles does it.  An enqueue.
void bring_home(fs_sim* s) {
    if (!s->key_in_pairs && !s->rho_in_rho2) return;
    launch_keys_from_pairs(s->stream, s->n, s->key_in_pairs ? s->pairs.p : nullptr, s->key.p, s->rho_in_rho2 ? s->rho2.p : nullptr,
                           s->rho.p);
    s->key_in_pairs = false; s->rho_in_rho2 = false;
}

// The count becomes new_n (2 <= new_n <= capacity, != n), the state arrays already hold it (or will, in stream order).  What
// every change shares: the queries and surface tension's forces no longer belong to the state, a registered hand-off's view is
// re-materialised on demand, and the bitonic sort's bookkeeping follows (sort_count_changed).  The counting sort keeps no word
// whose place depends on the count (its scratch is laid out by the capacity): it never waits.
fs_status count_changed(fs_sim* s, uint32_t new_n) {
    fs_status health = FS_OK;
    if (bitonic(s)) health = sort_count_changed(s->stream, s->sortp, s->sort_dirty, s->n, new_n);
    else s->sortp.touched();
    s->n = new_n;
    s->walk_ready = false;
    s->st.valid = false;
    s->dif.valid = false;
    s->aos_tick = 0xFFFFFFFFu;
    return health;
}

// The removal both forms end in: removal.flags (device, n bytes) and removal.sums are filled.  Blocking.
fs_status remove2(fs_sim* s, uint32_t* removed) {
    const uint32_t n = s->n, cap = s->capacity;
    uint32_t keep = 0;
    FS_TRY(removal_survivors(s->stream, s->removal, n, bitonic(s) ? &s->sortp : nullptr, s->sort_dirty.p, &keep));
    if (keep == n) return FS_OK;                          // nothing matched: nothing changes, queries stay valid
    bring_home(s);
    if (!s->aos.p) FS_HIP(s->aos.alloc(cap));
    // out of place: positions and velocities into the spare arrays (in bitonic mode the step swaps those two sets itself), pred,
    // rho and key into the AoS staging buffer (32 B per slot: cap float2, cap words, cap words) and back; ids and channels into
    // tracking's other set
    Compact2 C{};
    C.pos = s->pos.p; C.vel = s->vel.p; C.pred = s->pred.p; C.rho = (const uint32_t*)s->rho.p; C.key = s->key.p;
    C.pos_out = s->pos_s.p; C.vel_out = s->vel_s.p;
    C.pred_out = (float2*)s->aos.p; C.rho_out = (uint32_t*)(C.pred_out + cap); C.key_out = C.rho_out + cap;
    compact_tracking(&C, s->trk, cap);
    launch_remove_scatter(s->stream, n, s->removal.flags.p, s->removal.sums.p, C);
    FS_HIP(hipGetLastError());
    FS_HIP(hipMemcpyAsync(s->pred.p, C.pred_out, (size_t)keep * sizeof(float2), hipMemcpyDeviceToDevice, s->stream));
    FS_HIP(hipMemcpyAsync(s->rho.p, C.rho_out, (size_t)keep * 4, hipMemcpyDeviceToDevice, s->stream));
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

uint32_t fs_capacity(const fs_sim* s) { return s ? s->capacity : 0; }
uint32_t fs_track_next_id(const fs_sim* s) { return (s && s->trk.on()) ? s->trk.next_id : 0; }

fs_status fs_reserve(fs_sim* s, uint32_t capacity) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_INVALID, SLAB);
    if (capacity > MAX_SLOTS) return fail(FS_ERR_INVALID, "capacity > 2^28 (32-bit byte offsets)");
    if (s->aos_live) return fail(FS_ERR_INVALID, "reserve: a renderer hand-off is registered, the exported allocation cannot move (size the handle with fs_options.capacity)");
    if (capacity <= s->capacity) return FS_OK;
    FS_HIP(hipSetDevice(s->device));
    const size_t cap = capacity, n = s->n;
    const bool counting = s->opts.sort_mode == FS_SORT_COUNTING;
    // everything new first: on failure the locals go and the handle is what it was
    ParticleArrays A;                                       // pos .. pairs (and an 8-word counter that is dropped again)
    DevArray<uint32_t> key, dirty, csort;
    DevArray<fs_particle> aos;
    DevArray<float2> stf, fb;
    TrackingGrowth G;
    hipError_t e = hipSuccess;
    auto ok = [&e](hipError_t r) { e = r; return r == hipSuccess; };
    (void)(ok(A.alloc_common(cap)) && ok(key.alloc(cap)) && ok(dirty.alloc(sort_tile_count(capacity))) && ok(aos.alloc(cap)) &&
           ok(csort.alloc(counting ? counting_sort_scratch_words(capacity, s->ncell) : 0)) && ok(stf.alloc(s->st.stf.p ? cap : 0)) && ok(fb.alloc(s->dif.fb.p ? cap : 0)) &&
           ok(G.alloc(s->trk, cap)));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FS_ERR_OOM, "reserve: device arrays");
    }
    // Behind the steps in flight: the state, the last step's sorted arrays (the queries read pred, vel, rho / rho2 and pairs;
    // the keys may live in pairs, the densities in rho2) and forces, the sort's words.  The counting sort's scratch starts as at
    // create, all zero.  safe, fdefer, fwork and bbounds are written and read within one step: nothing to carry.
    hipStream_t q = s->stream;
    if (e == hipSuccess) e = hipMemsetAsync(dirty.p, 0, dirty.n * 4, q);
    if (e == hipSuccess) e = carry(q, dirty, s->sort_dirty, s->sort_dirty.n);   // tile flags and plan words keep their places: they follow n
    if (e == hipSuccess && csort.p) e = hipMemsetAsync(csort.p, 0, csort.n * 4, q);
    if (e == hipSuccess) e = carry(q, A.pos, s->pos, n);
    if (e == hipSuccess) e = carry(q, A.vel, s->vel, n);
    if (e == hipSuccess) e = carry(q, A.pos_s, s->pos_s, n);
    if (e == hipSuccess) e = carry(q, A.vel_s, s->vel_s, n);
    if (e == hipSuccess) e = carry(q, A.pred, s->pred, n);
    if (e == hipSuccess) e = carry(q, A.rho, s->rho, n);
    if (e == hipSuccess) e = carry(q, A.rho2, s->rho2, n);
    if (e == hipSuccess) e = carry(q, A.pairs, s->pairs, n);
    if (e == hipSuccess) e = carry(q, key, s->key, n);
    if (e == hipSuccess) e = carry(q, stf, s->st.stf, n);
    if (e == hipSuccess) e = carry(q, fb, s->dif.fb, n);
    if (e == hipSuccess) e = G.carry_from(q, s->trk, n, s->capacity, cap);
    const hipError_t es = hipStreamSynchronize(q);                         // before anything is freed, whatever happened
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(FS_ERR_DEVICE, hipGetErrorString(e));
    s->pos = std::move(A.pos); s->vel = std::move(A.vel); s->pos_s = std::move(A.pos_s); s->vel_s = std::move(A.vel_s);
    s->pred = std::move(A.pred); s->rho = std::move(A.rho); s->rho2 = std::move(A.rho2); s->safe = std::move(A.safe);
    s->fdefer = std::move(A.fdefer); s->fwork = std::move(A.fwork); s->bbounds = std::move(A.bbounds); s->pairs = std::move(A.pairs);
    s->key = std::move(key); s->sort_dirty = std::move(dirty); s->aos = std::move(aos);
    if (csort.p) s->csort = std::move(csort);
    if (stf.p) s->st.stf = std::move(stf);
    if (fb.p) s->dif.fb = std::move(fb);
    G.commit(s->trk);
    s->removal.release();                                                   // sized by the capacity: the next removal allocates it again
    s->capacity = capacity;
    return sort_health(s);
}

fs_status fs_emit_particles(fs_sim* s, const fs_particle* src, size_t n) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_INVALID, SLAB);
    if (n == 0) return FS_OK;
    if (!src) return fail(FS_ERR_INVALID, "null argument");
    if (n > (size_t)(s->capacity - s->n)) return fail(FS_ERR_INVALID, "emit: count + n exceeds the capacity (fs_reserve first)");
    FS_HIP(hipSetDevice(s->device));
    if (!s->aos.p) FS_HIP(s->aos.alloc(s->capacity));
    bring_home(s);
    // as fs_upload_particles stores them, at slot `count`: through the staging buffer's own slots [count, count + n), so that a
    // registered hand-off's view of the particles before them is not written over
    fs_particle* stage = s->aos.p + s->n;
    FS_HIP(hipMemcpyAsync(stage, src, n * sizeof(fs_particle), hipMemcpyHostToDevice, s->stream));
    launch_import_aos(s->stream, (uint32_t)n, stage, s->pos.p + s->n, s->pred.p + s->n, s->vel.p + s->n, s->rho.p + s->n, s->key.p + s->n);
    FS_HIP(hipGetLastError());
    s->trk.emitted(s->stream, s->n, (uint32_t)n, s->capacity);
    FS_HIP(hipStreamSynchronize(s->stream));               // `src` belongs to the caller again
    return count_changed(s, s->n + (uint32_t)n);
}

fs_status fs_emit_nozzle(fs_sim* s, const fs_nozzle* z) {
    static_assert(sizeof(fs_nozzle) == 40, "fs_nozzle is 40 bytes");
    if (!s || !z) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_INVALID, SLAB);
    const uint64_t m = (uint64_t)z->nu * z->nv;
    if (z->nu == 0u || z->nv == 0u || m > MAX_SLOTS) return fail(FS_ERR_INVALID, "nozzle: nu * nv must be 1 .. 2^28");
    const fs_vec2 f[4] = {z->origin, z->u, z->v, z->velocity};
    for (const fs_vec2& a : f)
        if (!std::isfinite(a.x) || !std::isfinite(a.y)) return fail(FS_ERR_INVALID, "nozzle: non-finite component");
    if (m > (uint64_t)(s->capacity - s->n)) return fail(FS_ERR_INVALID, "emit: count + nu * nv exceeds the capacity (fs_reserve first)");
    FS_HIP(hipSetDevice(s->device));
    bring_home(s);
    Nozzle2 Z;
    Z.origin = make_float2(z->origin.x, z->origin.y); Z.u = make_float2(z->u.x, z->u.y);
    Z.v = make_float2(z->v.x, z->v.y); Z.velocity = make_float2(z->velocity.x, z->velocity.y);
    Z.nu = z->nu; Z.nv = z->nv;
    launch_emit_nozzle(s->stream, Z, s->pos.p + s->n, s->pred.p + s->n, s->vel.p + s->n, s->rho.p + s->n, s->key.p + s->n);
    FS_HIP(hipGetLastError());
    s->trk.emitted(s->stream, s->n, (uint32_t)m, s->capacity);
    return count_changed(s, s->n + (uint32_t)m);
}

fs_status fs_remove_in_box(fs_sim* s, const fs_vec2* lo, const fs_vec2* hi, uint32_t* removed) {
    if (removed) *removed = 0;
    if (!s || !lo || !hi || !removed) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_INVALID, SLAB);
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(s->removal.reserve(s->capacity));
    launch_remove_box(s->stream, s->n, s->pos.p, make_float2(lo->x, lo->y), make_float2(hi->x, hi->y), s->removal.flags.p, s->removal.sums.p);
    return remove2(s, removed);
}

fs_status fs_remove_flagged(fs_sim* s, const uint8_t* flags, size_t n, uint32_t* removed) {
    if (removed) *removed = 0;
    if (!s || !flags || !removed) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_INVALID, SLAB);
    if (n != s->n) return fail(FS_ERR_INVALID, "removal: n must equal the particle count");
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(s->removal.reserve(s->capacity));
    FS_HIP(hipMemcpyAsync(s->removal.flags.p, flags, n, hipMemcpyHostToDevice, s->stream));
    launch_remove_count_flags(s->stream, s->n, s->removal.flags.p, s->removal.sums.p);
    return remove2(s, removed);
}

}  // extern "C"
