// engine_3d.hip — host side of the 3D extension of the step: the handle and the fs3_* C ABI (kernels and launchers:
// kernels_3d.hip, kernels_density3d.hip, kernels_force3d.hip; fs_3d.h).  From the 2D engine (engine.h): the device check, the create-time proofs, the owners and the
// sort policy.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "../../include/fluidsim.h"
#include "engine.h"
#include "fs_3d.h"

using fsd::DevArray;
using fsd::fail;
namespace {
void lattice3(const fs3_settings& st, fs_vec3 off, fs3_particle* dst, size_t n) {
    const uint32_t side = (uint32_t)std::llround(std::cbrt((double)st.particle_count));
    const float half = (float)side * 0.5f, s = st.particle_spacing;
    for (uint32_t i = 0; i < st.particle_count && i < n; ++i) {
        const uint32_t ix = i % side, iy = (i / side) % side, iz = i / (side * side);
        fs3_particle q;
        std::memset(&q, 0, sizeof q);
        q.position.x = ((float)ix - half + 0.5f) * s + off.x;
        q.position.y = ((float)iy - half + 0.5f) * s + off.y;
        q.position.z = ((float)iz - half + 0.5f) * s + off.z;
        q.predicted_position = q.position;
        dst[i] = q;
    }
}
}  // namespace

// Every resource is held by an owner (fs_host.h) and freed by `delete`; members go in reverse order of declaration: the
// device arrays first, then the events (profile ring, sort policy, t1 / t0), the stream last.
struct fs_sim3 {
    fs3_settings st{};
    uint32_t n = 0, gw = 0, gh = 0, gd = 0, ncell = 0, tick = 0, work_cap = 0;
    int device = 0;
    int math_mode = FS_MATH_IEEE;
    fsd::Stream stream;
    fsd::Event t0, t1;
    fsd::SortPolicy sortp;       // host side of the sort's late-stage plan (sort_policy.h)
    fsd::PassRing prof;          // per-pass timing
    DevArray<float4> pos, vel, pos_s, vel_s, pred;
    DevArray<uint32_t> key, cs, counter, dirty;
    DevArray<fsd::u64> pairs;
    DevArray<fsd::u64> masks;        // 9 x n pass masks of the 27-cell sweep, k3_density -> k3_force (Params3::handoff)
    bool handoff = true;
    DevArray<unsigned char> work;
    DevArray<fs3_particle> aos;
    fsd::ConstDiv div_2h3{}, div_h2{};
    bool share_div = false;      // all create-time proofs of the shared-denominator path succeeded
    float mass = 0.0f;           // of the tick of the last step enqueued: what field sampling weighs with
    bool sample_stale = true;    // no step enqueued since create / the last upload: records and cell table do not belong together
    // scratch of surface extraction, allocated by its first call and grown only by a larger lattice
    DevArray<float> mesh_field;      // node densities
    DevArray<uint32_t> mesh_rank;    // per node: the vertex index of its cell
    DevArray<uint32_t> mesh_sums;    // two words per workgroup of the count pass: sums, then offsets
    // the opt-in static collider: one float4 push vector per voxel; cw == 0: none, and never set: no allocation.
    // coll.n is the capacity (it only grows), cw * ch * cd the field in use
    DevArray<float4> coll;
    uint32_t cw = 0, ch = 0, cd = 0;
    // the opt-in surface tension: never enabled: no allocation, no launch
    struct Tension {
        DevArray<float4> st;         // the last step's force per sorted slot {x, y, z, 0}; allocated by the first enable
        float sigma = 0.0f, tau = 0.0f;
        bool on = false;
        bool valid = false;          // a step has been enqueued since the feature was last enabled: st belongs to the state
    } tension;
    // the opt-in particle tracking: the 2D engine's owner (engine.h), stride n; never enabled: no allocation, no launch
    fsd::Tracking trk;

    // the arrays as the launchers see them (fs_3d.h): the force pass writes the new positions into the spare buffer
    fsd::Arrays3 arrays() const {
        fsd::Arrays3 A;
        A.pos = pos.p; A.vel = vel.p; A.pos_out = pos_s.p; A.vel_s = vel_s.p; A.pred = pred.p; A.key = key.p;
        A.pairs = pairs.p; A.cs = cs.p; A.masks = handoff ? masks.p : nullptr;
        A.work = work.p; A.counter = counter.p; A.work_cap = work_cap; A.aos = aos.p;
        return A;
    }
};

static const float PI3 = 3.14159265359f;

// What the step and field sampling both need of Params3: counts, grid, h, the half-bounds and the poly6 constant; the rest zero.
static fsd::Params3 params3_common(const fs_sim3& s, float mass) {
    const float h = s.st.smoothing_radius;
    fsd::Params3 P;
    std::memset(&P, 0, sizeof P);
    P.n = s.n; P.gw = s.gw; P.gh = s.gh; P.gd = s.gd; P.ncell = s.ncell;
    P.h = h; P.h2 = h * h;
    P.bx = s.st.size.x * 0.5f; P.by = s.st.size.y * 0.5f; P.bz = s.st.size.z * 0.5f;
    P.mass = mass;
    P.poly6 = 315.0f / (64.0f * PI3 * std::pow(h, 9.0f));      // host libm, as in the oracle
    return P;
}

static fs_status enqueue3(fs_sim3* s, const fs3_tick_settings* t) {
    using namespace fsd;
    s->tick += 1;
    const float h = s->st.smoothing_radius;
    Params3 P = params3_common(*s, t->mass);
    P.dt = t->delta;
    P.spiky = 15.0f / (PI3 * std::pow(h, 5.0f));
    P.visc_k = 15.0f / (2.0f * PI3 * (h * h * h));
    P.pressure_k = t->pressure_constant; P.rest_density = t->rest_density; P.damping = t->damping_factor;
    P.visc_coeff = t->viscosity_coefficient;
    P.gx = t->gravity.x; P.gy = t->gravity.y; P.gz = t->gravity.z;
    P.frame = s->tick;
    P.div_2h3 = s->div_2h3;
    P.div_h2 = s->div_h2;
    // the classification bounds the pressure numerators by (1 + 2^-22) h spiky 2^39 <= 2^60 (fs_device.h)
    P.share_div = (s->share_div && h * P.spiky <= FS_HSPIKY_HI) ? 1 : 0;
    P.handoff = s->handoff ? 1 : 0;
    {   // chunks of ~1/128 of the blocks, at most 2^7 (8 M: 31 250 blocks, a z-plane of the cube is ~310): FS3_XCD_CHUNK_LOG2 overrides
        static const int forced = getenv("FS3_XCD_CHUNK_LOG2") ? atoi(getenv("FS3_XCD_CHUNK_LOG2")) : -1;
        const uint32_t nb = blocks3(s->n);
        uint32_t c = 0;
        while (c < 7u && (128u << (c + 1u)) <= nb) ++c;
        // 8 M, steps 10-110, strict / tolerance step (ms): c = 0: 3.329 / 2.732, 3: 3.277 / 2.675, 5: 3.260 / 2.645,
        // 7: 3.255 / 2.636, 8: 3.281 / 2.650, 10: 3.403 / 2.738, 12: 3.425 / 2.761 (large chunks bind an XCD to one depth)
        P.xcd_chunk_log2 = forced >= 0 ? (uint32_t)(forced > 16 ? 16 : forced) : c;
    }
    const bool tol = s->math_mode == FS_MATH_TOLERANCE;
    hipStream_t st = s->stream;
    hipEvent_t* ev = nullptr;
    if (s->prof.on) {
        const fs_status r = s->prof.begin();
        if (r != FS_OK) return r;
        ev = s->prof.current();
    }
    const Arrays3 A = s->arrays();
    FS_HIP(s->sortp.throttle());                           // at most SortPolicy::FLIGHT steps ahead of the device
    if (ev) FS_HIP(hipEventRecord(ev[0], st));
    // predict + key are fused into the first sort kernel (k_bitonic_local<true, 2, *>), as in 2D: no separate launch,
    // the unsorted pairs never touch HBM.  FS3_SEPARATE_KEYGEN=1 keeps the round-2 kernel (A/B measurements).
    static const bool separate_keygen = getenv("FS3_SEPARATE_KEYGEN") != nullptr;
    if (separate_keygen) launch3_predict_key(st, P, A);
    if (ev) FS_HIP(hipEventRecord(ev[1], st));
    fsd::SortPlan plan;
    if (!s->sortp.plan(s->n, &plan)) return fail(FS_ERR_DEVICE, "sort: the stand-by kernel's grid barrier timed out");
    if (separate_keygen) {
        launch_bitonic_sort(st, s->pairs.p, s->n, s->dirty.p, nullptr, &plan);
    } else {
        const fsd::KeyGen3 kg{P.dt, P.h, P.bx, P.by, P.bz, P.gw, P.gh};
        const fsd::SortKeys keys(kg, s->pos.p, s->vel.p, s->counter.p);
        launch_bitonic_sort(st, s->pairs.p, s->n, s->dirty.p, &keys, &plan);
    }
    if (ev) FS_HIP(hipEventRecord(ev[2], st));
    launch3_reorder(st, P, A);
    s->trk.carry(st, s->n, s->pairs.p, s->n);              // particle tracking, if on (inside the FS_PASS_REORDER interval)
    if (ev) FS_HIP(hipEventRecord(ev[3], st));
    launch3_density(st, P, A, tol);
    if (ev) FS_HIP(hipEventRecord(ev[4], st));
    // positions ping-pong: read the previous state (s->pos, source order) through the pairs, write the new one into s->pos_s
    // the step's completion event (sort_policy.h: the host stays at most four steps ahead) rides on the force kernel as its
    // completion signal — no marker packet behind it (engine.hip enqueue_step does the same); a profiled step records markers anyway
    hipEvent_t done = ev ? nullptr : s->sortp.flight_event();
    // the collider, if one is set, by value: this step keeps the field it was enqueued with (fs3_collider_* order their writes
    // on the stream behind it)
    const Collide3 K{s->coll.p, s->cw, s->ch, s->cd, s->st.size.x, s->st.size.y, s->st.size.z};
    // surface tension, if enabled: its pass between the density and the force pass (inside the force interval of the profile),
    // with the coefficients of this enqueue by value
    if (s->tension.on) {
        const Tension3 T{P.h2, 6.0f * P.poly6, 3.0f * P.h2, s->tension.sigma, s->tension.tau};
        launch3_surface_tension(st, P, A, T, s->tension.st.p);
        s->tension.valid = true;
    }
    launch3_force(st, P, A, tol, done, s->cw ? &K : nullptr, s->tension.on ? s->tension.st.p : nullptr);
    std::swap(s->pos, s->pos_s);
    s->mass = t->mass; s->sample_stale = false;
    if (ev) { FS_HIP(hipEventRecord(ev[5], st)); FS_HIP(hipEventRecord(ev[6], st)); /* FS_PASS_BOUNDARY: slab handles only */ s->prof.pending += 1; }
    if (ev) FS_HIP(s->sortp.step_enqueued(st));
    else s->sortp.step_bound();
    FS_HIP(hipGetLastError());
    return FS_OK;
}

extern "C" {

fs_status fs3_reference_lattice(const fs3_settings* st, fs_vec3 off, fs3_particle* dst, size_t n) {
    if (!st || (!dst && n)) return fail(FS_ERR_INVALID, "null argument");
    lattice3(*st, off, dst, n);
    return FS_OK;
}

fs_status fs3_create(const fs3_settings* st, int device, fs_vec3 off, fs_sim3** out) {
    return fs3_create_ex(st, device, off, FS_MATH_IEEE, out);
}

fs_status fs3_create_ex(const fs3_settings* st, int device, fs_vec3 off, int math_mode, fs_sim3** out) {
    if (!st || !out) return fail(FS_ERR_INVALID, "null argument");
    *out = nullptr;
    if (math_mode != FS_MATH_IEEE && math_mode != FS_MATH_TOLERANCE)
        return fail(FS_ERR_UNSUPPORTED, "3D math_mode must be FS_MATH_IEEE or FS_MATH_TOLERANCE");
    if (st->particle_count <= 1) return fail(FS_ERR_INVALID, "particle_count <= 1");
    if (st->particle_count > (1u << 28)) return fail(FS_ERR_INVALID, "particle_count > 2^28 (32-bit byte offsets)");
    if (!(st->smoothing_radius > 0.0f) || !(st->size.x > 0) || !(st->size.y > 0) || !(st->size.z > 0))
        return fail(FS_ERR_INVALID, "bad settings");
    const uint32_t side = (uint32_t)std::llround(std::cbrt((double)st->particle_count));
    if ((uint64_t)side * side * side != st->particle_count) return fail(FS_ERR_INVALID, "particle_count must be a cube");
    // cells per axis, the f32 quotient as in fsd::grid_dims; kept in doubles until their product is known to fit
    const auto cells = [st](float size) { return (double)std::ceil(size / st->smoothing_radius) + 2; };
    const double gw = cells(st->size.x), gh = cells(st->size.y), gd = cells(st->size.z);
    if (gw * gh * gd >= 4294967295.0) return fail(FS_ERR_INVALID, "grid does not fit u32 cell ids");
    FS_TRY(fsd::use_device(device));
    std::unique_ptr<fs_sim3> s(new (std::nothrow) fs_sim3());   // an error exit frees whatever the handle holds by then
    if (!s) return fail(FS_ERR_OOM, "host allocation failed");
    s->st = *st; s->n = st->particle_count; s->device = device; s->math_mode = math_mode;
    s->gw = (uint32_t)gw; s->gh = (uint32_t)gh; s->gd = (uint32_t)gd;
    s->ncell = s->gw * s->gh * s->gd;
    s->work_cap = s->ncell / 16u + 1024u;
    FS_HIP(hipStreamCreateWithFlags(&s->stream.h, hipStreamNonBlocking));
    const size_t n = s->n;
    FS_HIP(s->pos.alloc(n)); FS_HIP(s->vel.alloc(n)); FS_HIP(s->pos_s.alloc(n)); FS_HIP(s->vel_s.alloc(n)); FS_HIP(s->pred.alloc(n + FS_PRED_SLACK));
    FS_HIP(s->key.alloc(n)); FS_HIP(s->pairs.alloc(n)); FS_HIP(s->cs.alloc((size_t)s->ncell + 1)); FS_HIP(s->counter.alloc(4));
    FS_HIP(s->dirty.alloc(fsd::sort_tile_count((uint32_t)n))); FS_HIP(s->work.alloc((size_t)s->work_cap * fsd::gap_entry_size()));
    FS_HIP(s->aos.alloc(n));
    s->handoff = !(getenv("FS3_HANDOFF") && atoi(getenv("FS3_HANDOFF")) == 0);
    if (s->handoff) FS_HIP(s->masks.alloc(18 * (size_t)n));   // hi words, then the lo words of rows of 65 .. 128
    FS_HIP(hipEventCreate(&s->t0.h)); FS_HIP(hipEventCreate(&s->t1.h));
    FS_HIP(hipMemsetAsync(s->cs.p, 0, s->cs.n * 4, s->stream));
    FS_HIP(hipMemsetAsync(s->counter.p, 0, 16, s->stream));
    FS_HIP(hipMemsetAsync(s->dirty.p, 0, s->dirty.n * 4, s->stream));
    FS_HIP(s->sortp.init(5));         // a z-plane of the cube holds n^(2/3) particles: the moves are long, start at stage S - 5
    {
        std::vector<fs3_particle> host(n);
        lattice3(*st, off, host.data(), n);
        FS_HIP(hipMemcpyAsync(s->aos.p, host.data(), n * sizeof(fs3_particle), hipMemcpyHostToDevice, s->stream));
        fsd::launch3_import(s->stream, s->n, s->arrays());
        FS_HIP(hipStreamSynchronize(s->stream));
    }
    {   // the create-time proofs of the 2D engine (engine.h): the two constant divisions for this h, the lean reciprocal / square root
        const float hh = st->smoothing_radius;
        bool rcp_ok, sqrt_ok;
        FS_TRY(fsd::prove_constdiv(s->stream, s->counter.p + 1, 2.0f * hh * hh * hh, &s->div_2h3));
        FS_TRY(fsd::prove_constdiv(s->stream, s->counter.p + 1, hh * hh, &s->div_h2));
        FS_TRY(fsd::prove_rcp_sqrt(s->stream, s->counter.p + 1, &rcp_ok, &sqrt_ok));
        s->share_div = rcp_ok && sqrt_ok && s->div_2h3.ok && s->div_h2.ok && hh >= 0x1p-19f && hh <= 0x1p19f;
    }
    *out = s.release();
    return FS_OK;
}

void fs3_destroy(fs_sim3* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    delete s;
}

fs_status fs3_step(fs_sim3* s, const fs3_tick_settings* t) {
    if (!s || !t) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipSetDevice(s->device));
    return enqueue3(s, t);
}
// a barrier time-out of the sort's stand-by kernel leaves the particle order undefined: reported wherever state is handed over
static fs_status sort_health3(fs_sim3* s) { return s->sortp.health(s->dirty.p, s->n); }
fs_status fs3_sync(fs_sim3* s) { if (!s) return fail(FS_ERR_INVALID, "null"); FS_HIP(hipStreamSynchronize(s->stream)); return sort_health3(s); }
void* fs3_stream(const fs_sim3* s) { return s ? (void*)s->stream.h : nullptr; }
uint32_t fs3_tick_count(const fs_sim3* s) { return s ? s->tick : 0; }
uint32_t fs3_particle_count(const fs_sim3* s) { return s ? s->n : 0; }
fs_status fs3_grid_dims(const fs_sim3* s, uint32_t* w, uint32_t* h, uint32_t* d) {
    if (!s || !w || !h || !d) return fail(FS_ERR_INVALID, "null argument");
    *w = s->gw; *h = s->gh; *d = s->gd;
    return FS_OK;
}
fs_status fs3_download_particles(fs_sim3* s, fs3_particle* dst, size_t n) {
    if (!s || (!dst && n)) return fail(FS_ERR_INVALID, "null argument");
    if (n > s->n) n = s->n;
    FS_HIP(hipSetDevice(s->device));
    fsd::launch3_export(s->stream, s->n, s->arrays());
    if (n) FS_HIP(hipMemcpyAsync(dst, s->aos.p, n * sizeof(fs3_particle), hipMemcpyDeviceToHost, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    return sort_health3(s);
}
fs_status fs3_upload_particles(fs_sim3* s, const fs3_particle* src, size_t n) {
    if (!s || (!src && n)) return fail(FS_ERR_INVALID, "null argument");
    if (n > s->n) n = s->n;
    FS_HIP(hipSetDevice(s->device));
    if (n) FS_HIP(hipMemcpyAsync(s->aos.p, src, n * sizeof(fs3_particle), hipMemcpyHostToDevice, s->stream));
    if (n) fsd::launch3_import(s->stream, (uint32_t)n, s->arrays());
    FS_HIP(hipStreamSynchronize(s->stream));
    s->sortp.touched();
    if (n) s->sample_stale = true;
    return FS_OK;
}
fs_status fs3_timed_steps(fs_sim3* s, const fs3_tick_settings* t, uint32_t steps, double* ms_total) {
    if (!s || !t || !ms_total) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipSetDevice(s->device));
    FS_HIP(hipEventRecord(s->t0, s->stream));
    for (uint32_t k = 0; k < steps; ++k) { fs_status r = enqueue3(s, t); if (r != FS_OK) return r; }
    FS_HIP(hipEventRecord(s->t1, s->stream));
    FS_HIP(hipEventSynchronize(s->t1));
    float ms = 0;
    FS_HIP(hipEventElapsedTime(&ms, s->t0, s->t1));
    *ms_total = ms;
    return sort_health3(s);
}
fs_status fs3_profile_enable(fs_sim3* s, int enable) { if (!s) return fail(FS_ERR_INVALID, "null"); s->prof.on = enable != 0; return FS_OK; }
fs_status fs3_profile_read(fs_sim3* s, double ms[FS_PASS_COUNT], uint64_t* steps, int reset) {
    if (!s || !ms) return fail(FS_ERR_INVALID, "null argument");
    return s->prof.read(ms, steps, reset);
}

// ---- 3D colliders -------------------------------------------------------------------------------------
}  // extern "C"
namespace {
const uint32_t COLLIDER_MAX_EXTENT = 1024u;

// The checks the two setters share, in the order the header lists them (the handle first, by the caller).
fs_status collider3_check(const void* array, uint32_t w, uint32_t h, uint32_t d) {
    if (!array) return fail(FS_ERR_INVALID, "null argument");
    if (w == 0u || h == 0u || d == 0u || w > COLLIDER_MAX_EXTENT || h > COLLIDER_MAX_EXTENT || d > COLLIDER_MAX_EXTENT)
        return fail(FS_ERR_INVALID, "collider: an extent of 0 or above 1024");
    return FS_OK;
}

// Room for `voxels` vectors.  Allocates only when the field grew, and then only after the steps in flight — which read the old
// array — are done.  On failure the handle has no collider.
fs_status collider3_reserve(fs_sim3* s, size_t voxels) {
    if (voxels <= s->coll.n) return FS_OK;
    FS_HIP(hipStreamSynchronize(s->stream));
    s->cw = s->ch = s->cd = 0;
    if (s->coll.alloc(voxels) != hipSuccess) {
        (void)hipGetLastError();
        s->coll.release();
        return fail(FS_ERR_OOM, "collider: device field");
    }
    return FS_OK;
}

// The field in use as w * h * d fs_vec3 on the host.  Blocking.
fs_status collider3_read(fs_sim3* s, fs_vec3* dst) {
    const size_t voxels = (size_t)s->cw * s->ch * s->cd;
    std::unique_ptr<float4[]> host(new (std::nothrow) float4[voxels]);
    if (!host) return fail(FS_ERR_OOM, "host allocation failed");
    FS_HIP(hipMemcpyAsync(host.get(), s->coll.p, voxels * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    for (size_t k = 0; k < voxels; ++k) dst[k] = fs_vec3{host[k].x, host[k].y, host[k].z};
    return FS_OK;
}
}  // namespace
extern "C" {

fs_status fs3_collider_upload(fs_sim3* s, const fs_vec3* field, uint32_t w, uint32_t h, uint32_t d) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    FS_TRY(collider3_check(field, w, h, d));
    const size_t voxels = (size_t)w * h * d;
    std::unique_ptr<float4[]> host(new (std::nothrow) float4[voxels]);
    if (!host) return fail(FS_ERR_OOM, "host allocation failed");
    for (size_t k = 0; k < voxels; ++k) {
        const fs_vec3 f = field[k];
        if (!std::isfinite(f.x) || !std::isfinite(f.y) || !std::isfinite(f.z)) return fail(FS_ERR_INVALID, "collider: non-finite component");
        host[k] = make_float4(f.x, f.y, f.z, 0.0f);
    }
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(collider3_reserve(s, voxels));
    // on the stream: after the steps in flight, before the steps to come
    FS_HIP(hipMemcpyAsync(s->coll.p, host.get(), voxels * sizeof(float4), hipMemcpyHostToDevice, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    s->cw = w; s->ch = h; s->cd = d;
    return FS_OK;
}

fs_status fs3_collider_from_mask(fs_sim3* s, const uint8_t* mask, uint32_t w, uint32_t h, uint32_t d, fs_vec3* field_host) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    FS_TRY(collider3_check(mask, w, h, d));
    const size_t voxels = (size_t)w * h * d;
    bool any_free = false;
    for (size_t k = 0; k < voxels && !any_free; ++k) any_free = !(mask[k] > 128);
    if (!any_free) return fail(FS_ERR_INVALID, "collider: the mask has no free voxel");
    FS_HIP(hipSetDevice(s->device));
    DevArray<uint8_t> dmask;
    DevArray<uint32_t> near_x, near_xy;
    if (dmask.alloc(voxels) != hipSuccess || near_x.alloc(voxels) != hipSuccess || near_xy.alloc(voxels) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FS_ERR_OOM, "collider: device staging");
    }
    FS_TRY(collider3_reserve(s, voxels));
    fsd::ColliderMask3 Q;
    Q.mask = dmask.p; Q.w = w; Q.h = h; Q.d = d;
    Q.vx = s->st.size.x / (float)w; Q.vy = s->st.size.y / (float)h; Q.vz = s->st.size.z / (float)d;
    Q.near_x = near_x.p; Q.near_xy = near_xy.p; Q.field = s->coll.p;
    hipError_t e = hipMemcpyAsync(dmask.p, mask, voxels, hipMemcpyHostToDevice, s->stream);
    if (e == hipSuccess) { fsd::launch3_collider_from_mask(s->stream, Q); e = hipGetLastError(); }
    const hipError_t es = hipStreamSynchronize(s->stream);      // before the staging is freed, whatever happened
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) { s->cw = s->ch = s->cd = 0; return fail(FS_ERR_DEVICE, hipGetErrorString(e)); }
    s->cw = w; s->ch = h; s->cd = d;
    return field_host ? collider3_read(s, field_host) : FS_OK;
}

fs_status fs3_collider_clear(fs_sim3* s) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipSetDevice(s->device));
    FS_HIP(hipStreamSynchronize(s->stream));       // the steps in flight read the field
    s->cw = s->ch = s->cd = 0;
    s->coll.release();
    return FS_OK;
}

fs_status fs3_collider_dims(const fs_sim3* s, uint32_t* w, uint32_t* h, uint32_t* d) {
    if (!s || !w || !h || !d) return fail(FS_ERR_INVALID, "null argument");
    *w = s->cw; *h = s->ch; *d = s->cd;
    return FS_OK;
}

fs_status fs3_collider_download(fs_sim3* s, fs_vec3* dst, size_t n) {
    if (!s || !dst) return fail(FS_ERR_INVALID, "null argument");
    if (s->cw == 0u) return fail(FS_ERR_INVALID, "collider: none is set");
    if (n != (size_t)s->cw * s->ch * s->cd) return fail(FS_ERR_INVALID, "collider: n must be w * h * d");
    FS_HIP(hipSetDevice(s->device));
    return collider3_read(s, dst);
}

// ---- 3D surface tension -------------------------------------------------------------------------------
fs_status fs3_set_surface_tension(fs_sim3* s, int enable, float coefficient, float threshold) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    if (!enable) { s->tension.on = false; return FS_OK; }          // the two floats are not looked at
    if (std::isnan(coefficient)) return fail(FS_ERR_INVALID, "surface tension: coefficient is NaN");
    if (std::isnan(threshold)) return fail(FS_ERR_INVALID, "surface tension: threshold is NaN");
    if (!s->tension.st.p) {
        FS_HIP(hipSetDevice(s->device));
        if (s->tension.st.alloc(s->n) != hipSuccess) {
            (void)hipGetLastError();
            s->tension.st.release();
            return fail(FS_ERR_OOM, "surface tension: device array");
        }
    }
    if (!s->tension.on) s->tension.valid = false;                  // fs3_download_surface_tension waits for a step of this enable
    s->tension.on = true; s->tension.sigma = coefficient; s->tension.tau = threshold;
    return FS_OK;
}

int fs3_surface_tension_enabled(const fs_sim3* s) { return (s && s->tension.on) ? 1 : 0; }

fs_status fs3_surface_tension_params(const fs_sim3* s, float* coefficient, float* threshold) {
    if (!s || !coefficient || !threshold) return fail(FS_ERR_INVALID, "null argument");
    if (!s->tension.on) return fail(FS_ERR_INVALID, "surface tension: not enabled");
    *coefficient = s->tension.sigma; *threshold = s->tension.tau;
    return FS_OK;
}

fs_status fs3_download_surface_tension(fs_sim3* s, fs_vec3* dst, size_t n) {
    if (!s || !dst) return fail(FS_ERR_INVALID, "null argument");
    if (!s->tension.on) return fail(FS_ERR_INVALID, "surface tension: not enabled");
    if (!s->tension.valid) return fail(FS_ERR_INVALID, "surface tension: no step since surface tension was last enabled");
    if (n != s->n) return fail(FS_ERR_INVALID, "surface tension: n must equal the particle count");
    FS_HIP(hipSetDevice(s->device));
    std::unique_ptr<float4[]> host(new (std::nothrow) float4[n]);
    if (!host) return fail(FS_ERR_OOM, "host allocation failed");
    FS_HIP(hipMemcpyAsync(host.get(), s->tension.st.p, n * sizeof(float4), hipMemcpyDeviceToHost, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    for (size_t k = 0; k < n; ++k) dst[k] = fs_vec3{host[k].x, host[k].y, host[k].z};
    return sort_health3(s);
}

// ---- 3D particle tracking -----------------------------------------------------------------------------
fs_status fs3_track_enable(fs_sim3* s, int channels) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipSetDevice(s->device));
    return s->trk.enable(s->stream, s->n, s->n, channels);
}

fs_status fs3_track_disable(fs_sim3* s) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    s->trk.channels = -1;           // the arrays stay allocated until the handle is destroyed
    return FS_OK;
}

int fs3_track_channels(const fs_sim3* s) { return s ? s->trk.channels : -1; }

}  // extern "C"
namespace {
// ids (attr = false) or one channel, host <-> the arrays of the last enqueued step.  Blocking.
fs_status track3_copy(fs_sim3* s, int channel, bool attr, void* host, size_t n, bool upload) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(s->trk.copy(s->stream, s->n, s->n, channel, attr, host, n, upload));
    return upload ? FS_OK : sort_health3(s);
}
}  // namespace
extern "C" {

fs_status fs3_track_download_ids(fs_sim3* s, uint32_t* dst, size_t n) { return track3_copy(s, 0, false, dst, n, false); }
fs_status fs3_track_upload_ids(fs_sim3* s, const uint32_t* src, size_t n) { return track3_copy(s, 0, false, (void*)src, n, true); }
fs_status fs3_track_download_attr(fs_sim3* s, int channel, float* dst, size_t n) { return track3_copy(s, channel, true, dst, n, false); }
fs_status fs3_track_upload_attr(fs_sim3* s, int channel, const float* src, size_t n) { return track3_copy(s, channel, true, (void*)src, n, true); }

fs_status fs3_track_ids_device(fs_sim3* s, const uint32_t** out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    return s->trk.device_ptr(s->n, 0, false, (const void**)out);
}

fs_status fs3_track_attr_device(fs_sim3* s, int channel, const float** out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    return s->trk.device_ptr(s->n, channel, true, (const void**)out);
}

/* Off the step path: two downloads and a scatter on the host, so entries of dst that no id names are never written. */
fs_status fs3_download_particles_by_id(fs_sim3* s, fs3_particle* dst, size_t n) {
    if (!s || (!dst && n)) return fail(FS_ERR_INVALID, "null argument");
    if (!s->trk.on()) return fail(FS_ERR_INVALID, "tracking is off (enable it first)");
    std::vector<fs3_particle> rec;
    std::vector<uint32_t> ids;
    try { rec.resize(s->n); ids.resize(s->n); } catch (const std::bad_alloc&) { return fail(FS_ERR_OOM, "host staging"); }
    FS_TRY(fs3_download_particles(s, rec.data(), rec.size()));
    FS_TRY(fs3_track_download_ids(s, ids.data(), ids.size()));
    fsd::Tracking::scatter_by_id(ids, rec, dst, n);
    return FS_OK;
}

// ---- 3D field sampling --------------------------------------------------------------------------------
}  // extern "C"
namespace {
// Argument and state checks the three calls share, in the order the header lists them.  *go = false: n == 0, nothing to do.
fs_status sample3_check(fs_sim3* s, const void* points_or_view, size_t n, const void* out, bool* go) {
    *go = false;
    if (n == 0) return FS_OK;
    if (!points_or_view || !out) return fail(FS_ERR_INVALID, "null argument");
    if (n > ((size_t)1 << 28)) return fail(FS_ERR_INVALID, "sampling: more than 2^28 points");
    if (s->sample_stale) return fail(FS_ERR_INVALID, "sampling needs a step since create and since the last upload of particles");
    *go = true;
    return FS_OK;
}

// The view checks of the grid forms: *n = width * height * depth.
fs_status sample3_grid_size(const fs3_view* view, size_t* n) {
    if (!view) return fail(FS_ERR_INVALID, "null argument");
    const uint64_t wh = (uint64_t)view->width * view->height;
    if (wh == 0 || view->depth == 0 || wh > (1ull << 28) || wh * view->depth > (1ull << 28))
        return fail(FS_ERR_INVALID, "bad grid size");
    *n = (size_t)(wh * view->depth);
    return FS_OK;
}

// Enqueue the kernel on the simulation's stream.  points_dev == nullptr: the voxel centres of `view`.
fs_status sample3_enqueue(fs_sim3* s, const fs_vec3* points_dev, const fs3_view* view, size_t n, fs3_sample* out_dev) {
    static_assert(sizeof(fs3_sample) == 40 && sizeof(fs_vec3) == 12, "fs3_sample is 40 bytes, fs_vec3 three floats");
    const fsd::Params3 P = params3_common(*s, s->mass);
    fsd::Sample3Query Q;
    Q.n = (uint32_t)n;
    Q.points = (const float*)points_dev;
    if (view) {
        Q.wmin = make_float3(view->world_min.x, view->world_min.y, view->world_min.z);
        Q.wmax = make_float3(view->world_max.x, view->world_max.y, view->world_max.z);
        Q.width = view->width; Q.height = view->height; Q.depth = view->depth;
    }
    Q.out = out_dev;
    fsd::launch3_sample(s->stream, P, s->arrays(), Q);
    FS_HIP(hipGetLastError());
    return FS_OK;
}

// The blocking forms (fs_host.h staged_query): points == nullptr: the grid of `view`.
fs_status sample3_host(fs_sim3* s, const fs_vec3* points, const fs3_view* view, size_t n, fs3_sample* out) {
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(fsd::staged_query(s->stream, points, n, out, nullptr, 0, [&](const fs_vec3* dpts, fs3_sample* dout, float*) {
        return sample3_enqueue(s, dpts, points ? nullptr : view, n, dout);
    }));
    return sort_health3(s);
}
}  // namespace
extern "C" {

fs_status fs3_sample_points(fs_sim3* s, const fs_vec3* points, size_t n, fs3_sample* out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    bool go;
    const fs_status r = sample3_check(s, points, n, out, &go);
    if (r != FS_OK || !go) return r;
    return sample3_host(s, points, nullptr, n, out);
}

fs_status fs3_sample_points_device(fs_sim3* s, const fs_vec3* points_dev, size_t n, fs3_sample* out_dev) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    bool go;
    const fs_status r = sample3_check(s, points_dev, n, out_dev, &go);
    if (r != FS_OK || !go) return r;
    FS_HIP(hipSetDevice(s->device));
    return sample3_enqueue(s, points_dev, nullptr, n, out_dev);
}

fs_status fs3_sample_grid(fs_sim3* s, const fs3_view* view, fs3_sample* out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    size_t n;
    FS_TRY(sample3_grid_size(view, &n));
    bool go;
    const fs_status r = sample3_check(s, view, n, out, &go);
    if (r != FS_OK || !go) return r;
    return sample3_host(s, nullptr, view, n, out);
}

// ---- the tracking channels in 3D field sampling -------------------------------------------------------
}  // extern "C"
namespace {
// The checks of the three calls after the handle and (grid) the view, in the order the header lists them.  *go = false: n == 0.
fs_status sample3_attr_check(fs_sim3* s, const void* points_or_view, size_t n, const void* attr_out, bool* go) {
    *go = false;
    if (s->trk.channels <= 0) return fail(FS_ERR_INVALID, "sampling: the channels need tracking with at least one channel");
    return sample3_check(s, points_or_view, n, attr_out, go);
}

fs_status sample3_attr_enqueue(fs_sim3* s, const fs_vec3* points_dev, const fs3_view* view, size_t n, float* weight_dev, float* attr_dev) {
    fsd::Sample3AttrQuery Q;
    Q.n = (uint32_t)n;
    Q.points = (const float*)points_dev;
    if (view) {
        Q.wmin = make_float3(view->world_min.x, view->world_min.y, view->world_min.z);
        Q.wmax = make_float3(view->world_max.x, view->world_max.y, view->world_max.z);
        Q.width = view->width; Q.height = view->height; Q.depth = view->depth;
    }
    Q.channels = s->trk.channels;
    Q.attr = s->trk.channel(0, s->n); Q.attr_stride = s->n;
    Q.weight_out = weight_dev; Q.attr_out = attr_dev;
    fsd::launch3_sample_attr(s->stream, params3_common(*s, s->mass), s->arrays(), Q);
    FS_HIP(hipGetLastError());
    return FS_OK;
}

// The blocking forms: points == nullptr: the grid of `view`.  weight_out may be null.
fs_status sample3_attr_host(fs_sim3* s, const fs_vec3* points, const fs3_view* view, size_t n, float* weight_out, float* attr_out) {
    FS_HIP(hipSetDevice(s->device));
    FS_TRY(fsd::staged_query(s->stream, points, n, weight_out, attr_out, (size_t)s->trk.channels,
                             [&](const fs_vec3* dpts, float* dweight, float* dattr) {
                                 return sample3_attr_enqueue(s, dpts, points ? nullptr : view, n, dweight, dattr);
                             }));
    return sort_health3(s);
}
}  // namespace
extern "C" {

fs_status fs3_sample_attr_points(fs_sim3* s, const fs_vec3* points, size_t n, float* weight_out, float* attr_out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    bool go;
    const fs_status r = sample3_attr_check(s, points, n, attr_out, &go);
    if (r != FS_OK || !go) return r;
    return sample3_attr_host(s, points, nullptr, n, weight_out, attr_out);
}

fs_status fs3_sample_attr_points_device(fs_sim3* s, const fs_vec3* points_dev, size_t n, float* weight_out_dev, float* attr_out_dev) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    bool go;
    const fs_status r = sample3_attr_check(s, points_dev, n, attr_out_dev, &go);
    if (r != FS_OK || !go) return r;
    FS_HIP(hipSetDevice(s->device));
    return sample3_attr_enqueue(s, points_dev, nullptr, n, weight_out_dev, attr_out_dev);
}

fs_status fs3_sample_attr_grid(fs_sim3* s, const fs3_view* view, float* weight_out, float* attr_out) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    size_t n;
    FS_TRY(sample3_grid_size(view, &n));
    bool go;
    const fs_status r = sample3_attr_check(s, view, n, attr_out, &go);
    if (r != FS_OK || !go) return r;
    return sample3_attr_host(s, nullptr, view, n, weight_out, attr_out);
}

// ---- 3D surface rendering -----------------------------------------------------------------------------
}  // extern "C"
namespace {
// The checks of both calls, in the order the header lists them.
fs_status surface3_check(const fs_sim3* s, const fs3_camera* cam, const fs3_surface_params* sp, const void* out) {
    static_assert(sizeof(fs3_camera) == 64 && sizeof(fs3_surface_params) == 20 && sizeof(fs3_surface_hit) == 40, "3D surface rendering records");
    if (!s || !cam || !sp || !out) return fail(FS_ERR_INVALID, "null argument");
    const uint64_t wh = (uint64_t)cam->width * cam->height;
    if (wh == 0 || wh > (1ull << 26)) return fail(FS_ERR_INVALID, "bad image size");
    if (cam->reserved != 0) return fail(FS_ERR_INVALID, "camera: reserved must be 0");
    if (cam->orthographic != 0 && cam->orthographic != 1) return fail(FS_ERR_INVALID, "camera: orthographic must be 0 or 1");
    if (!std::isfinite(sp->iso) || !(sp->iso > 0.0f)) return fail(FS_ERR_INVALID, "surface params: iso must be finite and > 0");
    if (!std::isfinite(sp->t_near) || !(sp->t_near >= 0.0f)) return fail(FS_ERR_INVALID, "surface params: t_near must be finite and >= 0");
    if (!std::isfinite(sp->ds) || !(sp->ds > 0.0f)) return fail(FS_ERR_INVALID, "surface params: ds must be finite and > 0");
    if (sp->max_steps < 1u || sp->max_steps > 4096u) return fail(FS_ERR_INVALID, "surface params: max_steps must be 1 .. 4096");
    if (sp->refine > 24u) return fail(FS_ERR_INVALID, "surface params: refine must be 0 .. 24");
    if (s->sample_stale) return fail(FS_ERR_INVALID, "rendering needs a step since create and since the last upload of particles");
    return FS_OK;
}

fs_status surface3_enqueue(fs_sim3* s, const fs3_camera* cam, const fs3_surface_params* sp, fs3_surface_hit* out_dev) {
    const fsd::Params3 P = params3_common(*s, s->mass);
    fsd::Surface3Query Q;
    Q.eye = make_float3(cam->eye.x, cam->eye.y, cam->eye.z);
    Q.forward = make_float3(cam->forward.x, cam->forward.y, cam->forward.z);
    Q.right = make_float3(cam->right.x, cam->right.y, cam->right.z);
    Q.up = make_float3(cam->up.x, cam->up.y, cam->up.z);
    Q.width = cam->width; Q.height = cam->height; Q.orthographic = cam->orthographic;
    Q.iso = sp->iso; Q.t_near = sp->t_near; Q.ds = sp->ds; Q.max_steps = sp->max_steps; Q.refine = sp->refine;
    Q.out = out_dev;
    fsd::launch3_render_surface(s->stream, P, s->arrays(), Q);
    FS_HIP(hipGetLastError());
    return FS_OK;
}
}  // namespace
extern "C" {

fs_status fs3_render_surface(fs_sim3* s, const fs3_camera* cam, const fs3_surface_params* sp, fs3_surface_hit* out) {
    FS_TRY(surface3_check(s, cam, sp, out));
    FS_HIP(hipSetDevice(s->device));
    const size_t n = (size_t)cam->width * cam->height;
    FS_TRY(fsd::staged_query(s->stream, (const fs_vec3*)nullptr, n, out, nullptr, 0, [&](const fs_vec3*, fs3_surface_hit* dout, float*) {
        return surface3_enqueue(s, cam, sp, dout);
    }));
    return sort_health3(s);
}

fs_status fs3_render_surface_device(fs_sim3* s, const fs3_camera* cam, const fs3_surface_params* sp, fs3_surface_hit* out_dev) {
    FS_TRY(surface3_check(s, cam, sp, out_dev));
    FS_HIP(hipSetDevice(s->device));
    return surface3_enqueue(s, cam, sp, out_dev);
}

// ---- 3D surface extraction ----------------------------------------------------------------------------
}  // extern "C"
namespace {
// The checks of both calls, in the order the header lists them.
fs_status mesh3_check(const fs_sim3* s, const fs3_view* view, float iso, const void* verts, uint32_t vert_cap, const void* tris,
                      uint32_t tri_cap, const void* counts) {
    static_assert(sizeof(fs3_mesh_vertex) == 40, "fs3_mesh_vertex is 40 bytes");
    if (!s || !view || !counts) return fail(FS_ERR_INVALID, "null argument");
    if (view->width < 2u || view->height < 2u || view->depth < 2u) return fail(FS_ERR_INVALID, "bad lattice size: an extent < 2");
    const uint64_t wh = (uint64_t)view->width * view->height;
    if (wh > (1ull << 26) || wh * view->depth > (1ull << 26)) return fail(FS_ERR_INVALID, "bad lattice size: more than 2^26 nodes");
    if (!std::isfinite(iso) || !(iso > 0.0f)) return fail(FS_ERR_INVALID, "extraction: iso must be finite and > 0");
    if ((!verts && vert_cap) || (!tris && tri_cap)) return fail(FS_ERR_INVALID, "extraction: null array with a non-zero capacity");
    if (s->sample_stale) return fail(FS_ERR_INVALID, "extraction needs a step since create and since the last upload of particles");
    return FS_OK;
}

// The query of a checked call on the handle's scratch, which grows here and nowhere else.  hipFree of the arrays it replaces
// waits for the work that still reads them.
fs_status mesh3_query(fs_sim3* s, const fs3_view* view, float iso, fsd::Mesh3Query* Q) {
    const size_t nodes = (size_t)view->width * view->height * view->depth;
    if (nodes > s->mesh_field.n) {
        const hipError_t e1 = s->mesh_field.alloc(nodes), e2 = s->mesh_rank.alloc(nodes);
        const hipError_t e3 = s->mesh_sums.alloc(2 * (size_t)fsd::mesh3_workgroups((uint32_t)nodes));
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
            (void)hipGetLastError();
            s->mesh_field.release(); s->mesh_rank.release(); s->mesh_sums.release();
            return fail(FS_ERR_OOM, "extraction: device scratch");
        }
    }
    Q->wmin = make_float3(view->world_min.x, view->world_min.y, view->world_min.z);
    Q->wmax = make_float3(view->world_max.x, view->world_max.y, view->world_max.z);
    Q->width = view->width; Q->height = view->height; Q->depth = view->depth;
    Q->iso = iso;
    Q->field = s->mesh_field.p; Q->rank = s->mesh_rank.p; Q->sums = s->mesh_sums.p;
    return FS_OK;
}

// Vertices (which also leaves every active cell's rank for the faces), then faces: whatever part has room.
fs_status mesh3_emit(fs_sim3* s, const fsd::Mesh3Query& Q) {
    if (Q.vert_cap == 0u && Q.tri_cap == 0u) return FS_OK;
    fsd::launch3_mesh_verts(s->stream, params3_common(*s, s->mass), s->arrays(), Q);
    if (Q.tri_cap != 0u) fsd::launch3_mesh_faces(s->stream, Q);
    FS_HIP(hipGetLastError());
    return FS_OK;
}
}  // namespace
extern "C" {

fs_status fs3_extract_surface_device(fs_sim3* s, const fs3_view* view, float iso, fs3_mesh_vertex* verts_dev, uint32_t vert_cap,
                                     uint32_t* tris_dev, uint32_t tri_cap, uint32_t* counts_dev) {
    FS_TRY(mesh3_check(s, view, iso, verts_dev, vert_cap, tris_dev, tri_cap, counts_dev));
    FS_HIP(hipSetDevice(s->device));
    fsd::Mesh3Query Q;
    FS_TRY(mesh3_query(s, view, iso, &Q));
    Q.counts = counts_dev; Q.verts = verts_dev; Q.vert_cap = vert_cap; Q.tris = tris_dev; Q.tri_cap = tri_cap;
    fsd::launch3_mesh_count(s->stream, params3_common(*s, s->mass), s->arrays(), Q);
    return mesh3_emit(s, Q);
}

// Blocking: the counts first (field, count and scan passes), then what fits of either array through the staging helper.
fs_status fs3_extract_surface(fs_sim3* s, const fs3_view* view, float iso, fs3_mesh_vertex* verts, uint32_t vert_cap, uint32_t* tris,
                              uint32_t tri_cap, uint32_t counts[2]) {
    FS_TRY(mesh3_check(s, view, iso, verts, vert_cap, tris, tri_cap, counts));
    FS_HIP(hipSetDevice(s->device));
    fsd::Mesh3Query Q;
    FS_TRY(mesh3_query(s, view, iso, &Q));
    uint32_t vt[2] = {0u, 0u};
    FS_TRY(fsd::staged_query(s->stream, (const fs_vec3*)nullptr, 2, vt, nullptr, 0, [&](const fs_vec3*, uint32_t* dcounts, float*) {
        Q.counts = dcounts;
        fsd::launch3_mesh_count(s->stream, params3_common(*s, s->mass), s->arrays(), Q);
        FS_HIP(hipGetLastError());
        return FS_OK;
    }));
    const uint32_t nv = vt[0] < vert_cap ? vt[0] : vert_cap, nt = vt[1] < tri_cap ? vt[1] : tri_cap;
    Q.vert_cap = nv; Q.tri_cap = 0u;
    if (nv) {
        FS_TRY(fsd::staged_query(s->stream, (const fs_vec3*)nullptr, nv, verts, nullptr, 0, [&](const fs_vec3*, fs3_mesh_vertex* dverts, float*) {
            Q.verts = dverts;
            return mesh3_emit(s, Q);
        }));
    }
    if (nt) {
        Q.verts = nullptr; Q.vert_cap = 0u; Q.tri_cap = nt;
        FS_TRY(fsd::staged_query(s->stream, (const fs_vec3*)nullptr, 3 * (size_t)nt, tris, nullptr, 0, [&](const fs_vec3*, uint32_t* dtris, float*) {
            Q.tris = dtris;
            if (nv) { fsd::launch3_mesh_faces(s->stream, Q); FS_HIP(hipGetLastError()); return FS_OK; }   // the ranks are there
            return mesh3_emit(s, Q);
        }));
    }
    counts[0] = vt[0]; counts[1] = vt[1];
    return sort_health3(s);
}

}  // extern "C"
