// engine_3d.h — what the host files of the fs3_* C ABI share: the 3D simulation handle with the state of each of its features, the
// Params3 both the step and the queries start from, and the few helpers more than one of them needs.  The handle's files:
// engine_3d.hip (lattice, life cycle, step, getters, transfers, timing), engine_3d_features.hip (what the step enqueues for:
// colliders, moving bodies, surface tension, tracking), engine_3d_query.hip (everything behind sample_stale: sampling, rendering, extraction),
// engine_3d_count.hip (a particle count that changes at run time: reserve, emit, remove; what it shares with the 2D handle's
// engine_count.hip: engine_count.h), engine_3d_stats.hip (fluid diagnostics; the 2D engine's StatsScratch).  What the bodies and the collider's mask producer share with the 2D handle's
// engine_features.hip: engine_bodies.h.
// From the 2D engine (engine.h): the device check, the create-time proofs, the owners, the sort policy, Tracking, RemoveScratch
// and BodySlots.
#pragma once
#include <cmath>
#include <cstring>
#include <memory>
#include <new>

#include "engine.h"
#include "fs_3d.h"

// Every resource is held by an owner (fs_host.h) and freed by `delete`; members go in reverse order of declaration: the
// device arrays first, then the events (profile ring, sort policy, t1 / t0), the stream last.
struct fs_sim3 {
    fs3_settings st{};
    uint32_t n = 0;              // the live count: what every step and query works on
    uint32_t cap = 0;            // slots of every per-slot array (>= n; == n until fs3_reserve), the stride of masks and channels
    uint32_t gw = 0, gh = 0, gd = 0, ncell = 0, tick = 0, work_cap = 0;
    int device = 0;
    int math_mode = FS_MATH_IEEE;
    fsd::Stream stream;
    fsd::Event t0, t1;
    fsd::SortPolicy sortp;       // host side of the sort's late-stage plan (sort_policy.h)
    fsd::PassRing prof;          // per-pass timing
    fsd::DevArray<float4> pos, vel, pos_s, vel_s, pred;
    fsd::DevArray<uint32_t> key, cs, counter, dirty;
    fsd::DevArray<fsd::u64> pairs;
    fsd::DevArray<fsd::u64> masks;   // 18 x cap pass masks of the 27-cell sweep, k3_density -> k3_force (Params3::handoff)
    bool handoff = true;
    fsd::DevArray<unsigned char> work;
    fsd::DevArray<fs3_particle> aos;
    fsd::ConstDiv div_2h3{}, div_h2{};
    bool share_div = false;      // all create-time proofs of the shared-denominator path succeeded
    float mass = 0.0f;           // of the tick of the last step enqueued: what field sampling weighs with
    bool sample_stale = true;    // no step enqueued since create / the last upload: records and cell table do not belong together

    // The opt-in features' state, one struct and one line in enqueue3 each.
    // Scratch of surface extraction, allocated by its first call and grown only by a larger lattice.
    struct MeshScratch {
        fsd::DevArray<float> field;      // node densities
        fsd::DevArray<uint32_t> rank;    // per node: the vertex index of its cell
        fsd::DevArray<uint32_t> sums;    // two words per workgroup of the count pass: sums, then offsets
        // Room for a lattice of `nodes`: all three or none.  hipFree of the arrays it replaces waits for the work that still reads them.
        fs_status reserve(size_t nodes) {
            if (nodes <= field.n) return FS_OK;
            const hipError_t e1 = field.alloc(nodes), e2 = rank.alloc(nodes);
            const hipError_t e3 = sums.alloc(2 * (size_t)fsd::mesh3_workgroups((uint32_t)nodes));
            if (e1 == hipSuccess && e2 == hipSuccess && e3 == hipSuccess) return FS_OK;
            (void)hipGetLastError();
            field.release(); rank.release(); sums.release();
            return fsd::fail(FS_ERR_OOM, "extraction: device scratch");
        }
    } mesh;
    // The opt-in static collider: one float4 push vector per voxel; w == 0: none, and never set: no allocation.
    // field.n is the capacity (it only grows), w * h * d the field in use.
    struct Collider {
        fsd::DevArray<float4> field;
        uint32_t w = 0, h = 0, d = 0;
        size_t voxels() const { return (size_t)w * h * d; }
        void set(uint32_t w_, uint32_t h_, uint32_t d_) { w = w_; h = h_; d = d_; }
        void clear() { w = h = d = 0; }
        // Room for `count` vectors.  Allocates only when the field grew, and then only after the steps in flight on `st` — which
        // read the old array — are done.  On failure the handle has no collider.
        fs_status reserve(hipStream_t st, size_t count) {
            if (count <= field.n) return FS_OK;
            FS_HIP(hipStreamSynchronize(st));
            clear();
            if (field.alloc(count) != hipSuccess) {
                (void)hipGetLastError();
                field.release();
                return fsd::fail(FS_ERR_OOM, "collider: device field");
            }
            return FS_OK;
        }
        // What a step takes, by value into *K: it keeps the field it was enqueued with (fs3_collider_* order their writes on the
        // stream behind it).  Null: none is set.  size: the settings' box.
        const fsd::Collide3* for_step(fs_vec3 size, fsd::Collide3* K) const {
            *K = fsd::Collide3{field.p, w, h, d, size.x, size.y, size.z};
            return w ? K : nullptr;
        }
    } collider;
    // The opt-in moving bodies: per slot a voxel field over the body's own box and the motion the host last set;
    // w == 0: the slot is free, and never created: no allocation, no launch.
    struct BodySlot {
        fsd::DevArray<float4> field;
        uint32_t w = 0, h = 0, d = 0;
        fs_vec3 extent{};
        fs3_body_motion motion{};
        size_t voxels() const { return (size_t)w * h * d; }
    };
    struct Bodies : fsd::BodySlots<BodySlot, FS3_MAX_BODIES> {      // has, count, free_slot: engine.h
        using Slot = BodySlot;
        // Opt-in loads (fs3_body_loads_* in engine_3d_features.hip): eight words per body, the 2D handle's type.
        using Loads = fsd::BodyLoads<FS3_MAX_BODIES, fsd::BODY3_LOAD_WORDS>;
        Loads loads;
        // What a step takes, by value into *B: the fields and the motions as they are when it is enqueued, the slots in use in
        // ascending order (fs3_body_* order their writes and frees on the stream behind it); *M: the slot of each.  Null: no slot
        // is in use.
        const fsd::Bodies3* for_step(fsd::Bodies3* B, fsd::BodyLoadMap* M) const {
            uint32_t c = 0;
            for (uint32_t k = 0; k < FS3_MAX_BODIES; ++k) {
                const Slot& b = slot[k];
                if (!b.w) continue;
                const fs3_body_motion& m = b.motion;
                M->slot[c] = k;
                fsd::Body3& K = B->body[c++];
                K.field = b.field.p; K.w = b.w; K.h = b.h; K.d = b.d;
                K.ex = b.extent.x; K.ey = b.extent.y; K.ez = b.extent.z;
                K.hx = b.extent.x * 0.5f; K.hy = b.extent.y * 0.5f; K.hz = b.extent.z * 0.5f;
                K.cx = m.centre.x; K.cy = m.centre.y; K.cz = m.centre.z;
                for (int e = 0; e < 9; ++e) K.r[e] = m.rot[e];
                K.ux = m.velocity.x; K.uy = m.velocity.y; K.uz = m.velocity.z;
                K.wx = m.angular_velocity.x; K.wy = m.angular_velocity.y; K.wz = m.angular_velocity.z;
            }
            B->count = M->count = c;
            return c ? B : nullptr;
        }
        // This step's pass behind the force kernel; it carries `done` in that kernel's place.  Loads on: the pass's second form and
        // its fold, which carries `done`, and a step more for every slot in use.
        void enqueue(hipStream_t st, const fsd::Params3& P, const fsd::Arrays3& A, const fsd::Bodies3& B, const fsd::BodyLoadMap& M,
                     hipEvent_t done) {
            if (!loads.on) { fsd::launch3_bodies(st, P, A, B, done); return; }
            fsd::launch3_bodies_loads(st, P, A, B, M, loads.shards.p, loads.words.p, done);
            for (uint32_t k = 0; k < M.count; ++k) loads.steps[M.slot[k]] += 1u;
        }
    } bodies;
    // The opt-in surface tension: never enabled: no allocation, no launch.
    struct Tension {
        fsd::DevArray<float4> st;    // the last step's force per sorted slot {x, y, z, 0}; allocated by the first enable
        float sigma = 0.0f, tau = 0.0f;
        bool on = false;
        bool valid = false;          // a step has been enqueued since the feature was last enabled: st belongs to the state
        // This step's pass, between the density and the force pass (inside the force interval of the profile), with the coefficients
        // of this enqueue by value; returns what launch3_force adds, or null.
        const float4* enqueue(hipStream_t stream, const fsd::Params3& P, const fsd::Arrays3& A) {
            using fsd::Tension3;
            if (!on) return nullptr;
            const Tension3 T{P.h2, 6.0f * P.poly6, 3.0f * P.h2, sigma, tau};
            fsd::launch3_surface_tension(stream, P, A, T, st.p);
            valid = true;
            return st.p;
        }
    } tension;
    // The opt-in particle tracking: the 2D engine's owner (engine.h), stride cap; never enabled: no allocation, no launch.
    fsd::Tracking trk;
    fsd::RemoveScratch removal;  // scratch of a removal: the 2D engine's owner too
    fsd::StatsScratch stats;     // scratch of the fluid diagnostics (engine_3d_stats.hip): likewise
    // The opt-in diffusion and buoyancy of the tracking channels (fs3_set_diffusion / fs3_set_buoyancy in
    // engine_3d_features.hip): the host settings of the 2D handle's fsd::Diffusion (engine.h).  Host settings only, until a
    // buoyancy channel is first set: then `fb`, 16 B per slot.  Nothing set: no launch, no allocation.
    struct Diffusion {
        float kappa[FS_TRACK_MAX_CHANNELS] = {};   // conductivity per channel; 0: the channel does not diffuse
        int buoy = -1;                  // the buoyancy channel, -1: none
        float beta = 0.0f, reference = 0.0f;
        fsd::DevArray<float4> fb;       // per sorted slot: what the last buoyancy step handed the force pass (st + b, or b), .w = 0
        bool valid = false;             // a buoyancy step has been enqueued since the channel was last set (and the count has not changed)
        // fs3_track_enable / fs3_track_disable: every setting goes
        void clear() {
            for (float& k : kappa) k = 0.0f;
            buoy = -1; beta = reference = 0.0f;
            valid = false;
        }
        // This step's pass, after surface tension's and before the force launch: the diffusing channels are advanced in place
        // (through the spare tracking set, which is free once the carry has run, and one device-to-device copy per row back — behind
        // every launch: the buoyancy tail reads the value before the pass), and with a buoyancy channel the force launch's `stf`
        // operand becomes fb.  Returns that operand: stf itself when there is no buoyancy channel.
        const float4* enqueue(hipStream_t st, const fsd::Params3& P, const fsd::Arrays3& A, const fs3_tick_settings& t,
                              const fsd::Tracking& trk, uint32_t cap, const float4* stf) {
            if (!trk.on()) return stf;
            fsd::Diffuse3Plan D;
            for (int c = 0; c < trk.channels; ++c)
                if (kappa[c] != 0.0f) {
                    D.channel[D.count] = c;
                    D.g[D.count++] = (2.0f * kappa[c]) * t.delta;
                }
            if (buoy >= 0 && buoy < trk.channels) {
                D.buoyancy_channel = buoy;
                D.beta = beta; D.reference = reference;
                D.gravity_x = t.gravity.x; D.gravity_y = t.gravity.y; D.gravity_z = t.gravity.z;
            }
            if (!D.count && D.buoyancy_channel < 0) return stf;
            float* const cur = trk.attr[trk.cur].p;
            float* const spare = trk.attr[trk.cur ^ 1].p;
            fsd::launch3_diffuse(st, P, A, D, cur, spare, cap, stf, fb.p);
            for (int k = 0; k < D.count && P.n; ++k) {
                const size_t row = (size_t)D.channel[k] * cap;
                (void)hipMemcpyAsync(cur + row, spare + row, (size_t)P.n * sizeof(float), hipMemcpyDeviceToDevice, st);   // errors: the step's hipGetLastError
            }
            if (D.buoyancy_channel < 0) return stf;
            valid = true;
            return fb.p;
        }
    } diffusion;

    // the arrays as the launchers see them (fs_3d.h): the force pass writes the new positions into the spare buffer
    fsd::Arrays3 arrays() const {
        fsd::Arrays3 A;
        A.pos = pos.p; A.vel = vel.p; A.pos_out = pos_s.p; A.vel_s = vel_s.p; A.pred = pred.p; A.key = key.p;
        A.pairs = pairs.p; A.cs = cs.p; A.masks = handoff ? masks.p : nullptr;
        A.work = work.p; A.counter = counter.p; A.work_cap = work_cap; A.aos = aos.p;
        return A;
    }
};

namespace fsd {

static const float PI3 = 3.14159265359f;

// What the step and field sampling both need of Params3: counts, grid, h, the half-bounds and the poly6 constant; the rest zero.
inline Params3 params3_common(const fs_sim3& s, float mass) {
    const float h = s.st.smoothing_radius;
    Params3 P;
    std::memset(&P, 0, sizeof P);
    P.n = s.n; P.gw = s.gw; P.gh = s.gh; P.gd = s.gd; P.ncell = s.ncell;
    P.h = h; P.h2 = h * h;
    P.bx = s.st.size.x * 0.5f; P.by = s.st.size.y * 0.5f; P.bz = s.st.size.z * 0.5f;
    P.mass = mass;
    P.poly6 = 315.0f / (64.0f * PI3 * std::pow(h, 9.0f));      // host libm, as in the oracle
    return P;
}

// a barrier time-out of the sort's stand-by kernel leaves the particle order undefined: reported wherever state is handed over
inline fs_status sort_health3(fs_sim3* s) { return s->sortp.health(s->dirty.p, s->n); }

// The box and lattice of an fs3_view into any query that carries them (Sample3Query, Sample3AttrQuery, Mesh3Query).
template <class Query>
void set_view3(Query* Q, const fs3_view& view) {
    Q->wmin = make_float3(view.world_min.x, view.world_min.y, view.world_min.z);
    Q->wmax = make_float3(view.world_max.x, view.world_max.y, view.world_max.z);
    Q->width = view.width; Q->height = view.height; Q->depth = view.depth;
}

// n float4 {x, y, z, -} of a device array as fs_vec3 on the host.  Blocking on `st`.
inline fs_status download_vec3(hipStream_t st, const float4* dev, size_t n, fs_vec3* dst) {
    std::unique_ptr<float4[]> host(new (std::nothrow) float4[n]);
    if (!host) return fail(FS_ERR_OOM, "host allocation failed");
    FS_HIP(hipMemcpyAsync(host.get(), dev, n * sizeof(float4), hipMemcpyDeviceToHost, st));
    FS_HIP(hipStreamSynchronize(st));
    for (size_t k = 0; k < n; ++k) dst[k] = fs_vec3{host[k].x, host[k].y, host[k].z};
    return FS_OK;
}

}  // namespace fsd
