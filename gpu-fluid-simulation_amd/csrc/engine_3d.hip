// engine_3d.hip — host side of the 3D extension of the step (kernels and launchers: kernels_3d.hip, kernels_density3d.hip,
// kernels_force3d.hip; fs_3d.h): the lattice, the handle's life cycle, the step, the getters, the particle transfers and the
// timed steps.  The handle and what its files share: engine_3d.h.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <vector>

#include "engine_3d.h"

using fsd::fail;
using fsd::sort_health3;
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

fs_status enqueue3(fs_sim3* s, const fs3_tick_settings* t) {
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
    s->trk.carry(st, s->n, s->pairs.p, s->cap);             // particle tracking, if on (inside the FS_PASS_REORDER interval)
    if (ev) FS_HIP(hipEventRecord(ev[3], st));
    launch3_density(st, P, A, tol);
    if (ev) FS_HIP(hipEventRecord(ev[4], st));
    // positions ping-pong: read the previous state (s->pos, source order) through the pairs, write the new one into s->pos_s
    // the step's completion event (sort_policy.h: the host stays at most four steps ahead) rides on the force kernel as its
    // completion signal — no marker packet behind it (engine.hip enqueue_step does the same); a profiled step records markers anyway
    hipEvent_t done = ev ? nullptr : s->sortp.flight_event();
    // the opt-in features' operands (engine_3d.h): the collider by value, and surface tension's pass ahead of the force pass
    Collide3 K;
    const float4* stf = s->tension.enqueue(st, P, A);
    stf = s->diffusion.enqueue(st, P, A, *t, s->trk, s->cap, stf);   // channel diffusion and buoyancy, if set
    // with moving bodies their pass follows the force kernel and carries the completion event in its place; with
    // their loads on (§26) that is the pass's loads form and its fold
    Bodies3 BD;
    fsd::BodyLoadMap BM{};
    const Bodies3* bodies = s->bodies.for_step(&BD, &BM);
    launch3_force(st, P, A, tol, bodies ? nullptr : done, s->collider.for_step(s->st.size, &K), stf);
    if (bodies) s->bodies.enqueue(st, P, A, *bodies, BM, done);
    std::swap(s->pos, s->pos_s);
    s->mass = t->mass; s->sample_stale = false;
    if (ev) { FS_HIP(hipEventRecord(ev[5], st)); FS_HIP(hipEventRecord(ev[6], st)); /* FS_PASS_BOUNDARY: slab handles only */ s->prof.pending += 1; }
    if (ev) FS_HIP(s->sortp.step_enqueued(st));
    else s->sortp.step_bound();
    FS_HIP(hipGetLastError());
    return FS_OK;
}
}  // namespace

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
    s->st = *st; s->n = s->cap = st->particle_count; s->device = device; s->math_mode = math_mode;
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

}  // extern "C"
