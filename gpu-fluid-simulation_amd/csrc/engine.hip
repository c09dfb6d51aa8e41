// engine.hip — host side of the C ABI (include/fluidsim.h), the core: the simulation handle's life cycle, SoA device state,
// the pass chain of one step on one HIP stream, the particle / start-index / force-field transfers and the renderer hand-off.
// What a handle offers beyond that: engine_features.hip, engine_query.hip, engine_selftest.hip; slab handles: engine_slab.hip.
//
// Mirrors FluidSimulation::{new,tick,accessors} (src/simulation.rs:139-564).
// There is no CPU fallback: every entry point that computes requires a HIP device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "engine.h"

static_assert(sizeof(fs_particle) == 32, "ParticleInstance is 32 bytes (src/simulation.rs:126-135)");
static_assert(offsetof(fs_particle, predicted_position) == 8 && offsetof(fs_particle, velocity) == 16 &&
                  offsetof(fs_particle, density) == 24 && offsetof(fs_particle, grid) == 28,
              "ParticleInstance offsets");
static_assert(sizeof(fs_uniform) == 120, "SimulationUniform is 120 bytes (src/simulation.rs:53-90)");
static_assert(offsetof(fs_uniform, gravity) == 16 && offsetof(fs_uniform, smoothing_radius) == 40 &&
                  offsetof(fs_uniform, poly6_kernel_volume) == 72 && offsetof(fs_uniform, mouse_state) == 92 &&
                  offsetof(fs_uniform, grid_w) == 104 && offsetof(fs_uniform, texture_size) == 112,
              "SimulationUniform offsets");

static thread_local std::string g_err;
namespace fsd { void set_last_error(const std::string& msg) { g_err = msg; } }   // fs_host.h: fail()
using namespace fsd;
namespace {

const float PI_F = 3.14159265359f;   // funcs.wgsl:54 == std::f32::consts::PI in f32

// Rust f32::powi (llvm.powi -> compiler-rt __powisf2): square-and-multiply.
float powi_f32(float a, int b) {
    float r = 1.0f;
    const bool recip = b < 0;
    for (;;) {
        if (b & 1) r *= a;
        b /= 2;
        if (b == 0) break;
        a *= a;
    }
    return recip ? 1.0f / r : r;
}

void host_lattice(const fs_settings& s, fs_vec2 off, fs_particle* dst, size_t n) {
    // src/simulation.rs:147-163 — f32 arithmetic exactly as written.
    const uint32_t count = s.particle_count;
    const float per_row = std::sqrt((float)count);
    const float per_col = ((float)count - 1.0f) / per_row + 1.0f;
    const size_t per_row_trunc = (size_t)per_row;
    for (uint32_t i = 0; i < count && (size_t)i < n; ++i) {
        const size_t col = (size_t)i % per_row_trunc;
        fs_particle q;
        std::memset(&q, 0, sizeof q);
        q.position.x = ((float)col - per_row * 0.5f + 0.5f) * s.particle_spacing + off.x;
        q.position.y = (std::floor((float)i / per_row) - per_col * 0.5f + 0.5f) * s.particle_spacing + off.y;
        q.predicted_position = q.position;
        dst[i] = q;
    }
}

}  // namespace

// ---- shared with the other engine files (engine.h) -----------------------------------------------------------------------
// src/simulation.rs:140-141
void fsd::grid_dims(const fs_settings& s, uint32_t* gw, uint32_t* gh) {
    *gw = (uint32_t)((size_t)std::ceil(s.size.x / s.smoothing_radius) + 2);
    *gh = (uint32_t)((size_t)std::ceil(s.size.y / s.smoothing_radius) + 2);
}

bool fsd::settings_valid(const fs_settings& s, std::string* why) {
    if (s.particle_count <= 1) { *why = "particle_count <= 1 (reference panics in ilog2, src/simulation.rs:323-324)"; return false; }
    if (s.particle_count > (1u << 28)) { *why = "particle_count > 2^28 (the kernels use 32-bit byte offsets into 8-byte arrays)"; return false; }
    if (!(s.smoothing_radius > 0.0f) || !std::isfinite(s.smoothing_radius)) { *why = "smoothing_radius must be finite and > 0"; return false; }
    if (!(s.size.x > 0.0f) || !(s.size.y > 0.0f) || !std::isfinite(s.size.x) || !std::isfinite(s.size.y)) { *why = "size must be finite and > 0"; return false; }
    if (!std::isfinite(s.particle_spacing)) { *why = "particle_spacing must be finite"; return false; }
    const double gw = std::ceil((double)s.size.x / s.smoothing_radius) + 2, gh = std::ceil((double)s.size.y / s.smoothing_radius) + 2;
    if (gw * gh >= 4294967295.0) { *why = "grid_w*grid_h does not fit u32 cell ids"; return false; }
    if ((double)s.texture_size.x * s.texture_size.y >= 4294967295.0) { *why = "texture too large"; return false; }
    return true;
}

void fsd::host_uniform(const fs_settings& s, const fs_tick_settings& t, uint32_t tick, fs_uniform* u) {
    // src/simulation.rs:470-497
    const float h = s.smoothing_radius;
    std::memset(u, 0, sizeof *u);
    u->delta = t.delta;
    u->particle_count = s.particle_count;
    u->sqr_radius = h * h;
    u->frame_time = tick;
    u->gravity = t.gravity;
    u->bounds = s.size;
    u->mouse_pos = t.mouse_pos;
    u->smoothing_radius = h;
    u->particle_mass = t.mass;
    u->pressure_constant = t.pressure_constant;
    u->rest_density = t.rest_density;
    u->damping_factor = t.damping_factor;
    u->viscosity_coefficient = t.viscosity_coefficient;
    u->surface_tension_treshold = t.surface_tension_treshold;
    u->surface_tension_coefficient = t.surface_tension_coefficient;
    const float h8 = powi_f32(h, 8);
    u->poly6_kernel_volume = 4.0f / (PI_F * h8);
    u->poly6_kernel_derivative = 24.0f / (PI_F * h8);
    u->poly6_kernel_laplacian = 8.0f / (PI_F * h8);
    u->spiky_kernel_derivative = 12.0f / (powi_f32(h, 4) * PI_F);
    u->viscosity_kernel = 15.0f / (2.0f * PI_F * powi_f32(h, 3));
    u->mouse_state = t.mouse_state;
    u->mouse_force_radius = t.mouse_force_radius;
    u->mouse_force_power = t.mouse_force_power;
    grid_dims(s, &u->grid_w, &u->grid_h);
    u->texture_size.x = (float)s.texture_size.x;
    u->texture_size.y = (float)s.texture_size.y;
}

StepParams fsd::make_params(const fs_sim& s, const fs_uniform& u, uint32_t own_lo, uint32_t own_hi) {
    StepParams P;
    std::memset(&P, 0, sizeof P);
    P.n = s.n;
    P.grid_w = s.grid_w; P.grid_h = s.grid_h; P.ncell = s.ncell;
    P.dt = u.delta;
    P.h = u.smoothing_radius;
    P.sqr_radius = u.sqr_radius;
    P.bounds_x = u.bounds.x; P.bounds_y = u.bounds.y;
    P.bs_x = u.bounds.x * 0.5f; P.bs_y = u.bounds.y * 0.5f;
    P.mass = u.particle_mass;
    // funcs.wgsl:76 — `4.0 / (PI * pow(h, 8.0))`: loop-invariant, evaluated once per tick on
    // the host with libm powf (the device pow is not correctly rounded).
    P.poly6_norm = 4.0f / (PI_F * std::pow(u.smoothing_radius, 8.0f));
    P.pressure_k = u.pressure_constant; P.rest_density = u.rest_density;
    P.damping = u.damping_factor; P.visc_coeff = u.viscosity_coefficient;
    P.spiky = u.spiky_kernel_derivative; P.visc_k = u.viscosity_kernel;
    P.gx = u.gravity.x; P.gy = u.gravity.y;
    P.mouse_x = u.mouse_pos.x; P.mouse_y = u.mouse_pos.y;
    P.mouse_radius = u.mouse_force_radius; P.mouse_power = u.mouse_force_power;
    P.mouse_state = u.mouse_state;
    P.frame_time = u.frame_time;
    P.tex_w = u.texture_size.x; P.tex_h = u.texture_size.y;
    P.tex_w_u = s.settings.texture_size.x;   // u32(u.texture_size.x), compute.wgsl:129
    P.tex_len = (uint32_t)s.tex.n;
    P.tex_zero = s.tex_zero ? 1 : 0;
    {   // xcd_block(): chunks of ~1/64 of the strips, at most 256 blocks (8 grid rows of the 16M scene), at least 1
        static const int forced = getenv("FS_XCD_CHUNK_LOG2") ? atoi(getenv("FS_XCD_CHUNK_LOG2")) : -1;
        const uint32_t nb = (s.capacity + 255u) / 256u;
        uint32_t c = 0;
        while (c < 8u && (64u << (c + 1u)) <= nb) ++c;
        P.xcd_chunk_log2 = forced >= 0 ? (uint32_t)forced : c;
    }
    P.ref_quirks = s.opts.ref_quirks;
    P.fast_math = s.opts.math_mode == FS_MATH_WGSL_ULP ? 1 : s.opts.math_mode == FS_MATH_TOLERANCE ? 2 : 0;
    P.div_2h3 = s.div_2h3;
    P.div_h2 = s.div_h2;
    P.div_h = s.div_h;
    // div_by_rcp's guards assume dst <= ~h <= 2^19 (fs_device.h); FS_NO_SHAREDIV=1 keeps every `/` a true division
    static const bool no_sharediv = getenv("FS_NO_SHAREDIV") != nullptr;
    // ... and the per-particle "safe operand" classification bounds the pressure numerators only if h * spiky <= 2^19
    const float hspiky = std::fabs(P.h * P.spiky);
    // ... and force_terms_shared has no `dst <= h` test of its own: the scan's !(r2 > sqr_radius) decides it, which holds when
    // sqr_radius is RN(h * h) (fs_force_pair.h); a handle for which it is not keeps the true-division path, as with any failed proof
    const float hh = P.h * P.h;
    P.half_h = 0.5f * P.h;
    P.share_div = (!no_sharediv && s.div_2h3.ok && s.div_h2.ok && s.rcp_ok && s.sqrt_ok && P.h >= 0x1p-19f && P.h <= 0x1p19f &&
                   hspiky <= FS_HSPIKY_HI && P.sqr_radius == hh) ? 1 : 0;
    P.col_origin = 0;
    P.own_lo = 0; P.own_hi = s.grid_w;
    P.grid_w_global = s.grid_w;
    P.n_live = nullptr;
    if (s.slab) {
        // local window: 1 padding + 2 ghost columns each side of [own_lo, own_hi)
        P.grid_w = own_hi - own_lo + 6u;
        P.ncell = P.grid_w * s.grid_h;
        P.col_origin = (int32_t)own_lo - 3;
        P.own_lo = own_lo; P.own_hi = own_hi;
        P.n = s.capacity;
        P.n_live = s.slab->counters.p;
        P.ref_quirks = 0;   // the global stale-start quirk cannot exist per rank (§8e)
        // the serial step advances every owned column in its one force launch; the overlapped step narrows this per launch
        P.adv_lo = P.own_lo; P.adv_hi = P.own_hi; P.adv_outside = 0;
        P.transposed = s.slab->transposed ? 1 : 0;
    }
    P.grid_u = P.transposed ? P.grid_h : P.grid_w;
    P.grid_v = P.transposed ? P.grid_w : P.grid_h;
    static const bool no_bb = getenv("FS_NO_BLOCK_BOUNDS") != nullptr;      // A/B: every pass reduces its block bounds itself
    P.block_bounds = no_bb ? nullptr : s.bbounds.p;
    return P;
}

fs_status fsd::use_device(int device, fs_status out_of_range) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(FS_ERR_DEVICE, "no HIP device: the engine has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(out_of_range, "device ordinal out of range");
    FS_HIP(hipSetDevice(device));
    return FS_OK;
}

// Prove (exhaustively, on the device) that x / c == div_const_fast(x, c, RN(1/c)) for every f32 x.
fs_status fsd::prove_constdiv(hipStream_t st, uint32_t* scratch_word, float c, ConstDiv* out, float hi, bool enabled) {
    out->c = c;
    out->y = 1.0f / c;
    out->ok = 0;
    if (!(c > 4.0f * FS_CONSTDIV_MIN) || !std::isfinite(c) || !std::isfinite(out->y) || !enabled) return FS_OK;
    if (!(hi > 0.0f)) hi = c;                          // the force kernel's numerators: 2^-60 <= |x| <= c
    if (!(hi < 0x1p40f) || !(hi >= FS_CONSTDIV_MIN)) return FS_OK;
    uint32_t bad = 1;
    FS_HIP(hipMemsetAsync(scratch_word, 0, sizeof(uint32_t), st));
    fsd::launch_verify_constdiv(st, c, out->y, FS_CONSTDIV_MIN, hi, scratch_word);
    FS_HIP(hipMemcpyAsync(&bad, scratch_word, sizeof bad, hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    out->ok = bad == 0 ? 1 : 0;
    return FS_OK;
}

// the lean reciprocal / square root of the shared-denominator path, over their whole ranges
fs_status fsd::prove_rcp_sqrt(hipStream_t st, uint32_t* scratch_two_words, bool* rcp_ok, bool* sqrt_ok) {
    *rcp_ok = *sqrt_ok = false;
    if (getenv("FS_NO_SHAREDIV")) return FS_OK;
    uint32_t bad[2] = {1, 1};
    FS_HIP(hipMemsetAsync(scratch_two_words, 0, 2 * sizeof(uint32_t), st));
    launch_verify_unary(st, 0, FS_RCP_LO, FS_RCP_HI, scratch_two_words);
    launch_verify_unary(st, 1, FS_SQRT_LO, FS_SQRT_HI, scratch_two_words + 1);
    FS_HIP(hipMemcpyAsync(bad, scratch_two_words, sizeof bad, hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    *rcp_ok = bad[0] == 0;
    *sqrt_ok = bad[1] == 0;
    return FS_OK;
}

static fs_status prove_force_constants(fs_sim* s) {
    const float h = s->settings.smoothing_radius;
    const bool on = !getenv("FS_NO_CONSTDIV");     // (read by the 2D handles only)
    FS_TRY(prove_constdiv(s->stream, s->counter.p + 1, 2.0f * h * h * h, &s->div_2h3, 0.0f, on));   // funcs.wgsl:119
    FS_TRY(prove_constdiv(s->stream, s->counter.p + 1, h * h, &s->div_h2, 0.0f, on));
    // cell coordinates: (clamped position + half the bounds) / h, numerators 0 .. 2 bs (host_uniform: bs = size / 2 - ...)
    const float reach = 4.0f * fmaxf(fabsf(s->settings.size.x), fabsf(s->settings.size.y));
    FS_TRY(prove_constdiv(s->stream, s->counter.p + 1, h, &s->div_h, reach, on));
    return prove_rcp_sqrt(s->stream, s->counter.p + 1, &s->rcp_ok, &s->sqrt_ok);
}

// What fs_create_ex and fs_slab_create share, once settings, sort mode, capacity and grid are set: the streams and events,
// the arrays every handle has, and the zeroes the reference's buffers start with.
fs_status fsd::create_common(fs_sim* s) {
    FS_HIP(hipStreamCreateWithFlags(&s->stream.h, hipStreamNonBlocking));
    // The pre-registered general work can run beside the lean force kernel on a second stream (FS_SIDE_STREAM=1).
    // Measured at 16M: force 0.725 -> 0.711 ms in the bench window and 1.10 -> 0.99 ms in the dense regime, but every
    // launch of the following sort then pays ~1 us more behind the cross-stream join (sort 0.70 -> 0.73 ms): a net
    // loss in the bench window, so it is off by default.
    if (getenv("FS_SIDE_STREAM")) {
        FS_HIP(hipStreamCreateWithFlags(&s->side.h, hipStreamNonBlocking));
        FS_HIP(hipEventCreateWithFlags(&s->ev_fork.h, hipEventDisableTiming));
        FS_HIP(hipEventCreateWithFlags(&s->ev_join.h, hipEventDisableTiming));
    }
    FS_HIP(hipEventCreate(&s->t0.h));
    FS_HIP(hipEventCreate(&s->t1.h));
    FS_HIP(s->sortp.init(8));   // slab handles use the pinned words for the force pass's work report only (sort: per-stage plan)
    const size_t cap = s->capacity;
    FS_HIP(s->alloc_common(cap));
    FS_HIP(s->key.alloc(cap));
    FS_HIP(s->aos.alloc(cap));
    FS_HIP(s->sort_dirty.alloc(fsd::sort_tile_count((uint32_t)cap)));
    FS_HIP(hipMemsetAsync(s->sort_dirty.p, 0, s->sort_dirty.n * sizeof(uint32_t), s->stream));
    FS_HIP(s->cs.alloc((size_t)s->ncell + 1));
    FS_HIP(s->start_ref.alloc(s->ncell));
    FS_HIP(s->tex.alloc((size_t)s->settings.texture_size.x * s->settings.texture_size.y));
    FS_HIP(s->work.alloc((size_t)s->work_cap * fsd::gap_entry_size()));
    if (s->slab || s->opts.sort_mode == FS_SORT_COUNTING) {
        FS_HIP(s->csort.alloc(fsd::counting_sort_scratch_words((uint32_t)cap, s->ncell)));
        FS_HIP(hipMemsetAsync(s->csort.p, 0, s->csort.n * sizeof(uint32_t), s->stream));   // histogram / tickets: zero between steps
    }
    // wgpu zero-initialises buffers: start_indices (simulation.rs:204-209), force field (:213-218)
    FS_HIP(hipMemsetAsync(s->start_ref.p, 0, s->start_ref.n * sizeof(uint32_t), s->stream));
    FS_HIP(hipMemsetAsync(s->cs.p, 0, s->cs.n * sizeof(uint32_t), s->stream));
    if (s->tex.n) FS_HIP(hipMemsetAsync(s->tex.p, 0, s->tex.n * sizeof(float2), s->stream));
    FS_HIP(hipMemsetAsync(s->counter.p, 0, 8 * sizeof(uint32_t), s->stream));
    FS_HIP(hipMemsetAsync(s->rho.p, 0, cap * sizeof(float), s->stream));
    return FS_OK;
}

// ... and what both end with, after the initial state is in place: the create-time proofs and the uniform of tick 0.
fs_status fsd::create_finish(fs_sim* s) {
    FS_TRY(prove_force_constants(s));
    fs_tick_settings t0;
    std::memset(&t0, 0, sizeof t0);
    host_uniform(s->settings, t0, 0, &s->uniform);
    return FS_OK;
}

fs_status fsd::sort_health(fs_sim* s) {
    if (s->slab || s->opts.sort_mode != FS_SORT_BITONIC) return FS_OK;
    return s->sortp.health(s->sort_dirty.p, s->n);
}

static fs_status enqueue_step(fs_sim* s, const fs_tick_settings* t) {
    s->tick += 1;                                              // src/simulation.rs:460
    host_uniform(s->settings, *t, s->tick, &s->uniform);
    s->uniform.particle_count = s->n;
    StepParams P = make_params(*s, s->uniform);
    // reference-sort path: no sorted copy of the positions — the force pass takes its own particle's position from the
    // previous state through the pair's source index and writes the new state into the spare buffer (swapped below)
    static const bool pos_by_src_env = [] { const char* e = getenv("FS_POS_BY_SRC"); return e ? atoi(e) != 0 : true; }();
    const bool pos_by_src = pos_by_src_env && s->opts.sort_mode != FS_SORT_COUNTING;
    P.pos_by_src = pos_by_src ? 1 : 0;
    hipStream_t st = s->stream;
    const bool prof = s->prof.on;
    hipEvent_t* ev = nullptr;
    if (prof) {
        FS_TRY(s->prof.begin());
        ev = s->prof.current();
    }
    if (s->n == 0) return FS_OK;
    FS_HIP(s->sortp.throttle());                       // at most SortPolicy::FLIGHT steps ahead of the device

    if (prof) FS_HIP(hipEventRecord(ev[0], st));
    // predict + key are fused into the first sort kernel of either mode (no separate launch)
    const bool counting = s->opts.sort_mode == FS_SORT_COUNTING;
    if (prof) FS_HIP(hipEventRecord(ev[1], st));
    if (counting) {
        fsd::launch_counting_sort(st, P, s->capacity, s->pos.p, s->vel.p, s->cs.p, s->csort.p, s->counter.p, s->safe.p, s->tick);
    } else {
        fsd::SortPlan plan;
        if (!s->sortp.plan(s->n, &plan)) return fail(FS_ERR_DEVICE, "sort: the stand-by kernel's grid barrier timed out");
        const fsd::SortKeys keys(P, s->pos.p, s->vel.p, s->counter.p);
        fsd::launch_bitonic_sort(st, s->pairs.p, s->n, s->sort_dirty.p, &keys, &plan);
    }
    if (prof) FS_HIP(hipEventRecord(ev[2], st));
    fsd::StepArrays A = s->step_arrays();
    s->key_in_pairs = true;        // the 4 B / particle of a second copy of the keys stay unwritten
    A.key_s = nullptr;
    if (pos_by_src) A.pos_s = nullptr;     // ... and so does the sorted copy of the positions
    if (counting)      // rank fix-up of the counting sort fused with the reorder pass (kernels_csort.hip)
        fsd::launch_counting_reorder(st, P, s->capacity, A);
    else
        fsd::launch_reorder(st, P, A, s->work_cap);
    s->trk.carry(st, s->n, s->pairs.p, s->capacity);     // particle tracking, if on (inside the FS_PASS_REORDER interval)
    if (prof) FS_HIP(hipEventRecord(ev[3], st));
    // strict / ulp modes: rho2.x IS the density; the separate 4-byte copy is only written in tolerance mode (rho2 = {P, 1/rho})
    s->rho_in_rho2 = P.fast_math != 2;
    if (s->rho_in_rho2) A.rho = nullptr;
    fsd::launch_density(st, P, A);
    if (prof) FS_HIP(hipEventRecord(ev[4], st));
    fsd::ForceLaunch L = s->force_launch();
    L.st_in = s->st.enqueue(st, P, A, s->uniform);       // surface tension, if on (inside the FS_PASS_FORCE interval)
    L.st_in = s->dif.enqueue(st, P, A, s->uniform, s->trk, s->capacity, L.st_in);   // channel diffusion and buoyancy, if set (likewise)
    A.rho = s->rho.p;                  // (the force kernels take the array whatever the mode)
    if (pos_by_src) { A.pos_s = s->pos.p; A.pos_out = s->pos_s.p; }    // the role swap described above
    if (s->aos_live) L.aos_out = s->aos.p;
    // with moving bodies their pass follows the force launches and carries the completion event in their place
    const bool bodies = s->bodies.count() != 0u;
    hipEvent_t done = prof ? nullptr : s->sortp.flight_event();
    if (!bodies) L.done = done;
    L.quad_entries = s->sortp.quad_entries();
    fsd::launch_force(st, P, A, L);
    if (bodies) s->bodies.enqueue(st, P, A, L.aos_out, done);   // on the buffers that hold the new state, before the role swap below
    if (pos_by_src) std::swap(s->pos, s->pos_s);   // the spare buffer now holds the state
    s->walk_ready = true;
    if (s->aos_live) s->aos_tick = s->tick;
    if (prof) {
        FS_HIP(hipEventRecord(ev[5], st));
        FS_HIP(hipEventRecord(ev[6], st));             // FS_PASS_BOUNDARY: slab handles only
        s->prof.pending += 1;
    }
    if (prof) FS_HIP(s->sortp.step_enqueued(st));      // (the profile's own events are markers anyway)
    else s->sortp.step_bound();                        // the general force launch (with bodies: theirs) carried the step's completion event
    FS_HIP(hipGetLastError());
    return FS_OK;
}

extern "C" {

int fs_abi_version(void) { return FS_ABI_VERSION; }
const char* fs_last_error(void) { return g_err.c_str(); }

void fs_options_default(fs_options* o) {
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->device = 0;
    o->sort_mode = FS_SORT_BITONIC;
    o->ref_quirks = 1;
}

fs_status fs_create(const fs_settings* settings, int device, fs_sim** out) {
    fs_options o;
    fs_options_default(&o);
    o.device = device;
    return fs_create_ex(settings, &o, out);
}

fs_status fs_create_ex(const fs_settings* settings, const fs_options* opts, fs_sim** out) {
    if (!settings || !opts || !out) return fail(FS_ERR_INVALID, "null argument");
    *out = nullptr;
    std::string why;
    if (!settings_valid(*settings, &why)) return fail(FS_ERR_INVALID, why);
    if (opts->sort_mode != FS_SORT_BITONIC && opts->sort_mode != FS_SORT_COUNTING)
        return fail(FS_ERR_INVALID, "unknown sort_mode");
    if (opts->math_mode != FS_MATH_IEEE && opts->math_mode != FS_MATH_WGSL_ULP && opts->math_mode != FS_MATH_TOLERANCE)
        return fail(FS_ERR_INVALID, "unknown math_mode");
    FS_TRY(use_device(opts->device));

    std::unique_ptr<fs_sim> s(new (std::nothrow) fs_sim());     // an error exit frees whatever the handle holds by then
    if (!s) return fail(FS_ERR_OOM, "host allocation failed");
    s->settings = *settings;
    s->opts = *opts;
    s->device = opts->device;
    s->n = settings->particle_count;
    s->capacity = opts->capacity > s->n ? opts->capacity : s->n;
    if (s->capacity > (1u << 28)) return fail(FS_ERR_INVALID, "capacity > 2^28");
    grid_dims(*settings, &s->grid_w, &s->grid_h);
    s->ncell = s->grid_w * s->grid_h;
    s->work_cap = s->ncell / 16u + 1024u;
    FS_TRY(create_common(s.get()));
    FS_HIP(hipMemsetAsync(s->key.p, 0, s->capacity * sizeof(uint32_t), s->stream));

    // initial lattice (simulation.rs:147-163) -> AoS staging -> SoA
    {
        std::vector<fs_particle> host(s->n);
        host_lattice(*settings, opts->initial_offset, host.data(), host.size());
        FS_HIP(hipMemcpyAsync(s->aos.p, host.data(), host.size() * sizeof(fs_particle), hipMemcpyHostToDevice, s->stream));
        fsd::launch_import_aos(s->stream, s->n, s->aos.p, s->pos.p, s->pred.p, s->vel.p, s->rho.p, s->key.p);
        FS_HIP(hipStreamSynchronize(s->stream));
    }
    FS_TRY(create_finish(s.get()));
    *out = s.release();
    return FS_OK;
}

void fs_destroy(fs_sim* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    if (void* comm = fs_slab_comm_stream(s)) (void)hipStreamSynchronize((hipStream_t)comm);   // an exchange / edge chain still in flight reads this handle's buffers
    delete s;
}

fs_status fs_step(fs_sim* s, const fs_tick_settings* t) {
    if (!s || !t) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_INVALID, "slab handle: use fs_slab_pack / fs_slab_step");
    FS_HIP(hipSetDevice(s->device));
    return enqueue_step(s, t);
}

fs_status fs_sync(fs_sim* s) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipStreamSynchronize(s->stream));
    FS_TRY(slab_sync(s));
    return sort_health(s);
}

uint32_t fs_tick_count(const fs_sim* s) { return s ? s->tick : 0; }
uint32_t fs_particle_count(const fs_sim* s) { return s ? s->n : 0; }
void* fs_stream(const fs_sim* s) { return s ? (void*)s->stream : nullptr; }

fs_status fs_grid_dims(const fs_sim* s, uint32_t* gw, uint32_t* gh) {
    if (!s || !gw || !gh) return fail(FS_ERR_INVALID, "null argument");
    *gw = s->grid_w; *gh = s->grid_h;
    return FS_OK;
}

fs_status fs_particles_device(fs_sim* s, const fs_particle** out) {
    if (!s || !out) return fail(FS_ERR_INVALID, "null argument");
    FS_JOIN(s);
    FS_HIP(hipSetDevice(s->device));
    if (!s->aos.p) FS_HIP(s->aos.alloc(s->capacity));
    if (!(s->aos_live && s->aos_tick == s->tick && s->tick != 0)) {   // live view: the force pass already wrote it
        fsd::launch_export_aos(s->stream, s->n, s->pos.p, s->pred.p, s->vel.p, s->rho.p, s->key.p, s->aos.p,
                               s->key_in_pairs ? s->pairs.p : nullptr, s->rho_in_rho2 ? s->rho2.p : nullptr);
        FS_HIP(hipGetLastError());
        if (s->aos_live) s->aos_tick = s->tick;
    }
    *out = s->aos.p;
    return FS_OK;
}

fs_status fs_start_indices_device(fs_sim* s, const uint32_t** out, size_t* count) {
    if (!s || !out) return fail(FS_ERR_INVALID, "null argument");
    FS_JOIN(s);
    *out = s->start_ref.p;
    if (count) *count = s->start_ref.n;
    return FS_OK;
}

fs_status fs_get_uniform(const fs_sim* s, fs_uniform* out) {
    if (!s || !out) return fail(FS_ERR_INVALID, "null argument");
    *out = s->uniform;
    return FS_OK;
}

fs_status fs_upload_force_field(fs_sim* s, const fs_vec2* field, uint32_t w, uint32_t h) {
    if (!s || !field) return fail(FS_ERR_INVALID, "null argument");
    FS_JOIN(s);
    if (w != s->settings.texture_size.x || h != s->settings.texture_size.y)
        return fail(FS_ERR_INVALID, "force field dimensions differ from settings.texture_size");
    FS_HIP(hipSetDevice(s->device));
    FS_HIP(hipMemcpyAsync(s->tex.p, field, (size_t)w * h * sizeof(fs_vec2), hipMemcpyHostToDevice, s->stream));
    bool zero = true;               // while the copy runs: does the field push anything at all? (`!= 0`: -0 is zero, NaN is not)
    for (size_t k = 0, m = (size_t)w * h; k < m && zero; ++k) zero = !(field[k].x != 0.0f) && !(field[k].y != 0.0f);
    FS_HIP(hipStreamSynchronize(s->stream));
    s->tex_zero = zero;
    return FS_OK;
}

fs_status fs_download_particles(fs_sim* s, fs_particle* dst, size_t n) {
    if (!s || (!dst && n)) return fail(FS_ERR_INVALID, "null argument");
    FS_JOIN(s);
    if (n > s->n) n = s->n;
    const fs_particle* dev = nullptr;
    FS_TRY(fs_particles_device(s, &dev));
    if (n) FS_HIP(hipMemcpyAsync(dst, dev, n * sizeof(fs_particle), hipMemcpyDeviceToHost, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    return sort_health(s);        // the records are in `dst` either way (diagnosis); FS_ERR_DEVICE says they are not to be trusted
}

fs_status fs_upload_particles(fs_sim* s, const fs_particle* src, size_t n) {
    if (!s || (!src && n)) return fail(FS_ERR_INVALID, "null argument");
    FS_JOIN(s);
    if (n > s->n) n = s->n;   // ResizableBuffer::write trims oversize data (src/buffer.rs:71-75)
    FS_HIP(hipSetDevice(s->device));
    if (!s->aos.p) FS_HIP(s->aos.alloc(s->capacity));
    if (n) FS_HIP(hipMemcpyAsync(s->aos.p, src, n * sizeof(fs_particle), hipMemcpyHostToDevice, s->stream));
    if (s->key_in_pairs || s->rho_in_rho2) {   // a partial upload keeps the other particles' keys / densities: bring them home first
        fsd::launch_keys_from_pairs(s->stream, s->n, s->key_in_pairs ? s->pairs.p : nullptr, s->key.p,
                                    s->rho_in_rho2 ? s->rho2.p : nullptr, s->rho.p);
        s->key_in_pairs = false; s->rho_in_rho2 = false;
    }
    fsd::launch_import_aos(s->stream, (uint32_t)n, s->aos.p, s->pos.p, s->pred.p, s->vel.p, s->rho.p, s->key.p);
    FS_HIP(hipStreamSynchronize(s->stream));
    s->aos_tick = 0xFFFFFFFFu;      // the live view (if any) no longer matches the state: re-materialise on demand
    s->sortp.touched();             // an arbitrary order: the per-stage launches stand by until reports pass again
    s->walk_ready = false;
    return FS_OK;
}

fs_status fs_download_start_indices(fs_sim* s, uint32_t* dst, size_t n) {
    if (!s || (!dst && n)) return fail(FS_ERR_INVALID, "null argument");
    FS_JOIN(s);
    if (n > s->start_ref.n) n = s->start_ref.n;
    FS_HIP(hipSetDevice(s->device));
    if (n) FS_HIP(hipMemcpyAsync(dst, s->start_ref.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    return FS_OK;
}

fs_status fs_upload_start_indices(fs_sim* s, const uint32_t* src, size_t n) {
    if (!s || (!src && n)) return fail(FS_ERR_INVALID, "null argument");
    FS_JOIN(s);
    if (n > s->start_ref.n) n = s->start_ref.n;
    FS_HIP(hipSetDevice(s->device));
    if (n) FS_HIP(hipMemcpyAsync(s->start_ref.p, src, n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    s->walk_ready = false;
    return FS_OK;
}

fs_status fs_reference_lattice(const fs_settings* settings, fs_vec2 offset, fs_particle* dst, size_t n) {
    if (!settings || (!dst && n)) return fail(FS_ERR_INVALID, "null argument");
    if (settings->particle_count == 0) return FS_OK;
    host_lattice(*settings, offset, dst, n);
    return FS_OK;
}

size_t fs_sort_schedule(uint32_t particle_count, fs_sort_step* dst, size_t cap) {
    // src/simulation.rs:323-347
    if (particle_count <= 1) return 0;
    uint32_t p2 = 1, stages = 0;
    while (p2 < particle_count) { p2 <<= 1; ++stages; }
    size_t k = 0;
    for (uint32_t stage = 0; stage < stages; ++stage)
        for (uint32_t step = 0; step <= stage; ++step, ++k)
            if (dst && k < cap) {
                const uint32_t gw = 1u << (stage - step);
                dst[k] = fs_sort_step{gw, 2 * gw - 1, step, particle_count};
            }
    return k;
}

fs_status fs_build_uniform(const fs_settings* settings, const fs_tick_settings* tick, uint32_t tick_count,
                           fs_uniform* out) {
    if (!settings || !tick || !out) return fail(FS_ERR_INVALID, "null argument");
    host_uniform(*settings, *tick, tick_count, out);
    return FS_OK;
}

fs_status fs_generate_force_field(fs_sim* s, int device, const uint8_t* image, uint32_t w, uint32_t h,
                                  fs_vec2* field_host) {
    if (!image || w == 0 || h == 0) return fail(FS_ERR_INVALID, "null/empty image");
    if (h > 1024 || w >= 65536) return fail(FS_ERR_UNSUPPORTED, "image larger than 65535 x 1024");
    if (s) {
        if (s->slab) return fail(FS_ERR_UNSUPPORTED, "force field on a slab handle");
        if (w != s->settings.texture_size.x || h != s->settings.texture_size.y)
            return fail(FS_ERR_INVALID, "image dimensions differ from settings.texture_size");
        device = s->device;
    }
    FS_TRY(use_device(device, FS_ERR_DEVICE));
    const size_t npix = (size_t)w * h;
    DevArray<unsigned char> dimg;
    DevArray<float> ddist;
    DevArray<uint32_t> dnear;
    DevArray<float2> dfield;        // without a handle: the field itself
    hipStream_t st = s ? s->stream : nullptr;
    hipError_t e = dimg.alloc(npix);
    if (e == hipSuccess) e = ddist.alloc(npix);
    if (e == hipSuccess) e = dnear.alloc(npix);
    if (e == hipSuccess && !s) e = dfield.alloc(npix);
    float2* out = s ? s->tex.p : dfield.p;
    if (s) s->tex_zero = false;     // produced on the device: contents unknown to the host
    if (e == hipSuccess) e = hipMemcpyAsync(dimg.p, image, npix, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) { fsd::launch_gradient_field(st, dimg.p, w, h, ddist.p, dnear.p, out); e = hipGetLastError(); }
    if (e == hipSuccess && field_host) e = hipMemcpyAsync(field_host, out, npix * sizeof(float2), hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);      // before the staging is freed, whatever happened
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(FS_ERR_DEVICE, hipGetErrorString(e));
    return FS_OK;
}

fs_status fs_profile_enable(fs_sim* s, int enable) {
    if (!s) return fail(FS_ERR_INVALID, "null argument");
    s->prof.on = enable != 0;
    return FS_OK;
}

fs_status fs_profile_read(fs_sim* s, double ms[FS_PASS_COUNT], uint64_t* steps, int reset) {
    if (!s || !ms) return fail(FS_ERR_INVALID, "null argument");
    FS_JOIN(s);
    return s->prof.read(ms, steps, reset);
}

fs_status fs_timed_steps(fs_sim* s, const fs_tick_settings* t, uint32_t steps, double* ms_total) {
    if (!s || !t || !ms_total) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_INVALID, "slab handle: use fs_slab_pack / fs_slab_step");
    FS_HIP(hipSetDevice(s->device));
    FS_HIP(hipEventRecord(s->t0, s->stream));
    for (uint32_t k = 0; k < steps; ++k) {
        FS_TRY(enqueue_step(s, t));
    }
    FS_HIP(hipEventRecord(s->t1, s->stream));
    FS_HIP(hipEventSynchronize(s->t1));
    float ms = 0.0f;
    FS_HIP(hipEventElapsedTime(&ms, s->t0, s->t1));
    *ms_total = ms;
    return sort_health(s);
}

/* ------------------------------------------------- renderer hand-off without a host round trip */
fs_status fs_export_handle(fs_sim* s, int which, fs_mem_handle* out) {
    if (!s || !out) return fail(FS_ERR_INVALID, "null argument");
    if (s->slab) return fail(FS_ERR_UNSUPPORTED, "export on a slab handle");
    if (which != FS_EXPORT_PARTICLES && which != FS_EXPORT_START_INDICES) return fail(FS_ERR_INVALID, "unknown export");
    FS_JOIN(s);
    FS_HIP(hipSetDevice(s->device));
    std::memset(out, 0, sizeof *out);
    void* base = nullptr;
    if (which == FS_EXPORT_PARTICLES) {
        if (!s->aos.p) FS_HIP(s->aos.alloc(s->capacity));
        if (!s->aos_live) {
            s->aos_live = true;                    // from now on k_force writes the records itself
            s->aos_tick = 0xFFFFFFFFu;
        }
        const fs_particle* dev = nullptr;          // make the view current for the state as it is now
        FS_TRY(fs_particles_device(s, &dev));
        base = s->aos.p;
        out->bytes = (uint64_t)s->n * sizeof(fs_particle);
    } else {
        base = s->start_ref.p;
        out->bytes = (uint64_t)s->start_ref.n * sizeof(uint32_t);
    }
    static_assert(sizeof(hipIpcMemHandle_t) <= sizeof(out->ipc), "fs_mem_handle.ipc too small");
    hipIpcMemHandle_t h;
    FS_HIP(hipIpcGetMemHandle(&h, base));
    std::memcpy(out->ipc, &h, sizeof h);
    out->device = s->device;
    out->dmabuf_fd = -1;
    // a dma-buf file descriptor of the same range, for consumers outside HIP (Vulkan / wgpu external memory);
    // optional: older runtimes lack the call, the IPC handle above is the portable path between HIP processes
    int fd = -1;
    if (hipMemGetHandleForAddressRange(&fd, base, (size_t)((out->bytes + 4095u) & ~(uint64_t)4095u), hipMemRangeHandleTypeDmaBufFd, 0) == hipSuccess)
        out->dmabuf_fd = fd;
    else
        (void)hipGetLastError();
    FS_HIP(hipStreamSynchronize(s->stream));
    return FS_OK;
}

fs_status fs_import_open(const fs_mem_handle* h, int device, void** ptr) {
    if (!h || !ptr) return fail(FS_ERR_INVALID, "null argument");
    *ptr = nullptr;
    FS_TRY(use_device(device, FS_ERR_DEVICE));
    hipIpcMemHandle_t ih;
    std::memcpy(&ih, h->ipc, sizeof ih);
    FS_HIP(hipIpcOpenMemHandle(ptr, ih, hipIpcMemLazyEnablePeerAccess));
    return FS_OK;
}

fs_status fs_import_read(const void* dev_ptr, size_t offset, void* dst, size_t bytes) {
    if (!dev_ptr || (!dst && bytes)) return fail(FS_ERR_INVALID, "null argument");
    FS_HIP(hipMemcpy(dst, (const char*)dev_ptr + offset, bytes, hipMemcpyDeviceToHost));
    return FS_OK;
}

fs_status fs_import_close(void* ptr) {
    if (!ptr) return FS_OK;
    FS_HIP(hipIpcCloseMemHandle(ptr));
    return FS_OK;
}

}  // extern "C"
