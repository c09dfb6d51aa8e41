// engine.h — what the host files of the C ABI share beyond fs_host.h: the 2D simulation handle and the state of each of its
// features, the step parameters, and the device check and create-time proofs (also used by the 3D handle's files through
// engine_3d.h).  The handle's files:
// engine.hip (life cycle, step, transfers, renderer hand-off), engine_features.hip (surface tension, particle tracking, channel diffusion, moving bodies;
// what the bodies share with the 3D handle's engine_3d_features.hip: engine_bodies.h, and BodySlots and BodyLoads below),
// engine_query.hip (density render, field sampling), engine_count.hip (a particle count that changes at run time; what it
// shares with the 3D handle's engine_3d_count.hip: engine_count.h, and Tracking and RemoveScratch below),
// engine_stats.hip (fluid diagnostics; what it shares with the 3D handle's engine_3d_stats.hip: StatsScratch below),
// engine_selftest.hip (self-tests, read-outs), engine_slab.hip (the multi-GPU slab handles).  Internal: include/fluidsim.h is the interface.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/fluidsim.h"
#include "fs_force_lists.h"
#include "fs_host.h"
#include "fs_kernels.h"
#include "sort_policy.h"

namespace fsd {

// The arrays one particle array's sort-reorder, density and force passes work on: the main array of every handle (fs_sim) and
// the boundary strip of an overlapped slab step (SlabState::Strip) each hold one set.
struct ParticleArrays {
    // SoA state.  pos/vel: current state (cell order of the last step).  *_s: the
    // cell-sorted snapshot the density/force passes read (Jacobi semantics).
    DevArray<float2> pos, vel, pos_s, vel_s, pred;
    DevArray<float> rho;
    DevArray<float2> rho2;          // {density, RN(1/density)}: what the force pass gathers per neighbour
    DevArray<uint32_t> fdefer, fwork;   // force pass: per-block deferred-wave bits and the worklist (fs_force_lists.h; its counters: counter[4..5])
    DevArray<uint32_t> bbounds;         // 8 words per 256-particle block: the density pass's block-wide sweep ranges, read by the force pass
    DevArray<unsigned long long> safe;   // one bit per sorted particle: coordinates / velocity inside the exact-quotient ranges (fs_device.h)
    DevArray<u64> pairs;
    DevArray<uint32_t> csort;       // scratch of the counting sort (FS_SORT_COUNTING)
    DevArray<uint32_t> cs;          // dense cell-start table, ncell+1
    DevArray<uint32_t> start_ref;   // reference start_indices (persistent, never cleared)
    DevArray<uint32_t> counter;     // the passes' work counters: from [0] the reorder's gap worklist, [4..5] the force pass
    DevArray<unsigned char> owned;  // slab mode

    // the arrays every handle and every strip has, for `cap` slots
    hipError_t alloc_common(size_t cap) {
        hipError_t e = hipSuccess;
        auto ok = [&e](hipError_t r) { e = r; return r == hipSuccess; };
        (void)(ok(pos.alloc(cap)) && ok(vel.alloc(cap)) && ok(pos_s.alloc(cap)) && ok(vel_s.alloc(cap)) &&
               ok(pred.alloc(cap + FS_PRED_SLACK)) && ok(rho.alloc(cap)) && ok(rho2.alloc(cap)) && ok(safe.alloc((cap + 63) / 64 + 1)) &&
               ok(fdefer.alloc(force_defer_words(cap))) && ok(fwork.alloc(force_worklist_words(cap))) &&
               ok(bbounds.alloc(8 * ((cap + 255) / 256 + 8))) && ok(pairs.alloc(cap)) && ok(counter.alloc(8)));
        return e;
    }
    // What the step launchers see of this set (fs_kernels.h); the force pass writes the new state over pos / vel.
    StepArrays step_arrays() const {
        StepArrays A;
        A.pos = pos.p; A.vel = vel.p; A.pos_s = pos_s.p; A.vel_s = vel_s.p; A.pred = pred.p;
        A.rho = rho.p; A.rho2 = rho2.p; A.pairs = pairs.p; A.cs = cs.p; A.start_ref = start_ref.p; A.safe = safe.p;
        A.fdefer = fdefer.p; A.fwork = fwork.p; A.fcount = counter.p + 4;
        A.pos_out = pos.p; A.vel_out = vel.p;
        A.owned = owned.p; A.csort = csort.p; A.counter = counter.p;
        return A;
    }
};

// Streams, events and the other things of a handle that are not device arrays.
struct HandleQueues {
    Stream stream;
    Stream side;                    // second stream of the force pass (general workgroups beside the lean kernel)
    Event ev_fork, ev_join;         // ... of `side`
    Event t0, t1;                   // fs_timed_steps
    SortPolicy sortp;               // host side of the sort's late-stage plan (sort_policy.h)
    PassRing prof;                  // per-pass timing (fs_host.h)
};

// The next step's messages, built by the edge columns' chain of an edge-first step into the send buffers of the last
// fs_slab_pack.  The next fs_slab_pack sends them as they are if nothing they depend on has changed since.
struct PrebuiltMessages {
    void *left = nullptr, *right = nullptr;   // the buffers the last fs_slab_pack was given (nullptr: no neighbour on that side)
    bool valid = false;                       // they hold the messages of tick + 1 ...
    float delta = 0.0f;                       // ... built with this delta
    uint32_t lo = 0, hi = 0;                  // ... and this owned window
    bool classified = false;                  // that chain also classified its particles' slots for the next pack (the histogram
                                              // counts it added stand until that pack, whether the messages are still valid or not)
    bool matches(const fs_slab_config& c, const void* send_left, const void* send_right, float d) const {
        return valid && left == (c.has_left ? send_left : nullptr) && right == (c.has_right ? send_right : nullptr) && delta == d &&
               lo == c.own_lo && hi == c.own_hi;
    }
    void invalidate() { valid = false; }
    void built(const fs_slab_config& c, float d) { valid = true; delta = d; lo = c.own_lo; hi = c.own_hi; }
};

// Opt-in surface tension (build extension; single-domain handles): fs_set_surface_tension, engine_features.hip.
struct SurfaceTension {
    DevArray<float2> stf;           // per sorted slot: the last ST step's force (allocated on first enable)
    bool on = false;
    bool valid = false;             // an ST step has been enqueued since create / since ST was last enabled
    // This step's pass, between the density and the force launches; returns what the force launch adds (ForceLaunch::st_in).
    const float2* enqueue(hipStream_t st, const StepParams& P, const StepArrays& A, const fs_uniform& u) {
        if (!on) return nullptr;
        launch_surface_tension(st, P, A, u.surface_tension_coefficient, u.surface_tension_treshold, u.poly6_kernel_derivative, stf.p);
        valid = true;
        return stf.p;
    }
};

// Opt-in particle tracking (build extension, DESIGN.md §12 and, on an fs_sim3, §20; single-domain handles): fs_track_* in
// engine_features.hip, fs3_track_* in engine_3d_features.hip.  Two sets that swap roles every step: [cur] holds the ids /
// channels in the order of the last enqueued step.  `capacity`: the slots of the handle, the stride of the channels (an fs_sim3: its cap).
struct Tracking {
    DevArray<uint32_t> id[2];
    DevArray<float> attr[2];        // channel c at c * capacity
    int channels = -1;              // -1: off
    int alloc_channels = 0;         // channels the attr arrays were allocated for
    int cur = 0;
    uint32_t next_id = 0;           // while on: the live count at enable, then + 1 per emitted particle, wrapping
    bool on() const { return channels >= 0; }
    // of the last enqueued step
    uint32_t* ids() const { return id[cur].p; }
    float* channel(int c, uint32_t capacity) const { return attr[cur].p + (size_t)c * capacity; }
    // ids / channels follow this step's permutation (`pairs`, after the reorder pass)
    void carry(hipStream_t st, uint32_t n, const u64* pairs, uint32_t capacity) {
        if (!on()) return;
        launch_track_carry(st, n, channels, pairs, id[cur].p, id[cur ^ 1].p, attr[cur].p, attr[cur ^ 1].p, capacity);
        cur ^= 1;
    }
    // Tracking's share of an emission of m records at slot `first`: the next m ids, +0.0f in every channel.
    void emitted(hipStream_t st, uint32_t first, uint32_t m, uint32_t capacity) {
        if (!on()) return;
        launch_emit_track(st, m, next_id, ids() + first, channels, channel(0, capacity) + first, capacity);
        next_id += m;               // wraps
    }
    // fs_track_enable / fs3_track_enable on the current device: allocates on first use, then id[i] = i and every channel +0.0f on
    // `st` — ordered after every step already enqueued, before every step enqueued from now on.
    fs_status enable(hipStream_t st, uint32_t n, uint32_t capacity, int ch) {
        if (ch < 0 || ch > FS_TRACK_MAX_CHANNELS) return fail(FS_ERR_INVALID, "tracking: channels must be in [0, FS_TRACK_MAX_CHANNELS]");
        if (!id[0].p) {
            for (int k = 0; k < 2; ++k)
                if (id[k].alloc(capacity) != hipSuccess) {
                    (void)hipGetLastError();
                    id[0].release(); id[1].release();
                    return fail(FS_ERR_OOM, "tracking: id arrays");
                }
        }
        if (ch > alloc_channels) {
            FS_HIP(hipStreamSynchronize(st));      // steps in flight may still read the arrays about to be replaced
            attr[0].release(); attr[1].release();
            alloc_channels = 0;
            for (int k = 0; k < 2; ++k)
                if (attr[k].alloc((size_t)ch * capacity) != hipSuccess) {
                    (void)hipGetLastError();
                    attr[0].release(); attr[1].release();
                    channels = -1;
                    return fail(FS_ERR_OOM, "tracking: channel arrays");
                }
            alloc_channels = ch;
        }
        cur = 0;
        launch_track_iota(st, n, ids());
        FS_HIP(hipGetLastError());
        if (ch && n) FS_HIP(hipMemsetAsync(attr[0].p, 0, (size_t)ch * capacity * sizeof(float), st));
        channels = ch;
        next_id = n;                // the ids in use are 0 .. n - 1: emission goes on from there
        return FS_OK;
    }
    // ids (is_attr = false) or one channel, host <-> the arrays of the last enqueued step, on the current device.  Blocking; the
    // caller reports the sort's health after a download.
    fs_status copy(hipStream_t st, uint32_t n, uint32_t capacity, int c, bool is_attr, void* host, size_t count, bool upload) {
        if (!host) return fail(FS_ERR_INVALID, "null argument");
        if (!on()) return fail(FS_ERR_INVALID, "tracking is off (enable it first)");
        if (is_attr && (c < 0 || c >= channels)) return fail(FS_ERR_INVALID, "tracking: no such channel");
        if (count != n) return fail(FS_ERR_INVALID, "tracking: n must equal the particle count");
        void* dev = is_attr ? (void*)channel(c, capacity) : (void*)ids();
        if (count) {
            if (upload) FS_HIP(hipMemcpyAsync(dev, host, count * 4, hipMemcpyHostToDevice, st));
            else FS_HIP(hipMemcpyAsync(host, dev, count * 4, hipMemcpyDeviceToHost, st));
        }
        FS_HIP(hipStreamSynchronize(st));
        return FS_OK;
    }
    // fs_track_ids_device / fs_track_attr_device (is_attr)
    fs_status device_ptr(uint32_t capacity, int c, bool is_attr, const void** out) const {
        if (!out) return fail(FS_ERR_INVALID, "null argument");
        if (!on()) return fail(FS_ERR_INVALID, "tracking is off (enable it first)");
        if (is_attr && (c < 0 || c >= channels)) return fail(FS_ERR_INVALID, "tracking: no such channel");
        *out = is_attr ? (const void*)channel(c, capacity) : (const void*)ids();
        return FS_OK;
    }
    // fs_download_particles_by_id's scatter on the host: dst[ids[i]] = rec[i] where ids[i] < n; other entries are never written
    template <class Rec>
    static void scatter_by_id(const std::vector<uint32_t>& ids, const std::vector<Rec>& rec, Rec* dst, size_t n) {
        for (size_t i = 0; i < ids.size(); ++i)
            if (ids[i] < n) dst[ids[i]] = rec[i];
    }
};

// Opt-in diffusion and buoyancy of the tracking channels (build extension; single-domain 2D handles):
// fs_set_diffusion / fs_set_buoyancy in engine_features.hip.  Host settings only, until a buoyancy channel is first set: then
// `fb`, 8 B per slot.  Nothing set: no launch, no allocation.
struct Diffusion {
    float kappa[FS_TRACK_MAX_CHANNELS] = {};   // conductivity per channel; 0: the channel does not diffuse
    int buoy = -1;                  // the buoyancy channel, -1: none
    float beta = 0.0f, reference = 0.0f;
    DevArray<float2> fb;            // per sorted slot: what the last buoyancy step handed the force pass (st + b, or b)
    bool valid = false;             // a buoyancy step has been enqueued since the channel was last set (and the count has not changed)
    // fs_track_enable / fs_track_disable: every setting goes
    void clear() {
        for (float& k : kappa) k = 0.0f;
        buoy = -1; beta = reference = 0.0f;
        valid = false;
    }
    // This step's pass, after surface tension's and before the force launches: the diffusing channels are advanced in place (through
    // the spare tracking set, which is free once the carry has run, and one device-to-device copy per row back), and with a buoyancy
    // channel the force launch's `st` operand becomes fb.  Returns that operand: st_in itself when there is no buoyancy channel.
    const float2* enqueue(hipStream_t st, const StepParams& P, const StepArrays& A, const fs_uniform& u, const Tracking& trk,
                          uint32_t capacity, const float2* st_in) {
        if (!trk.on()) return st_in;
        DiffusePlan D;
        for (int c = 0; c < trk.channels; ++c)
            if (kappa[c] != 0.0f) {
                D.channel[D.count] = c;
                D.g[D.count++] = (2.0f * kappa[c]) * u.delta;
            }
        if (buoy >= 0 && buoy < trk.channels) {
            D.buoyancy_channel = buoy;
            D.beta = beta; D.reference = reference;
            D.gravity_x = u.gravity.x; D.gravity_y = u.gravity.y;
        }
        if (!D.count && D.buoyancy_channel < 0) return st_in;
        float* const cur = trk.attr[trk.cur].p;
        float* const spare = trk.attr[trk.cur ^ 1].p;
        launch_diffuse(st, P, A, D, u.poly6_kernel_derivative, cur, spare, capacity, st_in, fb.p);
        for (int k = 0; k < D.count && P.n; ++k) {
            const size_t row = (size_t)D.channel[k] * capacity;
            (void)hipMemcpyAsync(cur + row, spare + row, (size_t)P.n * sizeof(float), hipMemcpyDeviceToDevice, st);   // errors: the step's hipGetLastError
        }
        if (D.buoyancy_channel < 0) return st_in;
        valid = true;
        return fb.p;
    }
};

// The slot table of the moving bodies of either handle (Bodies below, fs_sim3::Bodies in engine_3d.h): MAX slots of a type whose
// w == 0 says that the slot is free.
template <class Slot, uint32_t MAX>
struct BodySlots {
    Slot slot[MAX];
    bool has(uint32_t k) const { return k < MAX && slot[k].w != 0u; }
    uint32_t count() const { uint32_t c = 0; for (const Slot& b : slot) c += b.w ? 1u : 0u; return c; }
    // the lowest free slot, MAX when every slot is in use
    uint32_t free_slot() const { uint32_t k = 0; while (k < MAX && slot[k].w) ++k; return k; }
};

// The opt-in loads of either handle's bodies (fs_body_loads_* in engine_features.hip; fs3_body_loads_* in
// engine_3d_features.hip, §26) over MAX slots of WORDS 64-bit words.  words: MAX x WORDS by slot, what *_body_loads_device hands
// out; shards: the pass's scratch (BODY_LOAD_SHARDS rows of MAX x WORDS), zero between steps; both allocated by the first enable
// and kept for the life of the handle.  steps[k]: steps enqueued with loads on since slot k's words were last zeroed.  Each
// handle's file keeps its entry points, the order of its checks and its messages.
template <uint32_t MAX, uint32_t WORDS>
struct BodyLoads {
    bool on = false;
    DevArray<unsigned long long> words, shards;
    uint64_t steps[MAX] = {};
    static constexpr size_t SLOT_BYTES = WORDS * sizeof(unsigned long long);
    // Zeroes the words of `slot` on the stream, behind what is enqueued, and its step count (loads never enabled: no words).
    hipError_t zero(hipStream_t st, uint32_t slot) {
        steps[slot] = 0;
        return words.p ? hipMemsetAsync(words.p + slot * WORDS, 0, SLOT_BYTES, st) : hipSuccess;
    }
    // fs_body_loads_enable / fs3_body_loads_enable behind their checks (the device is set): on zeroes every slot, also when already on.
    fs_status enable(hipStream_t st, bool on_) {
        if (on_) {
            if (!words.p) {
                DevArray<unsigned long long> w, sh;
                if (w.alloc(MAX * WORDS) != hipSuccess || sh.alloc(BODY_LOAD_SHARDS * MAX * WORDS) != hipSuccess) {
                    (void)hipGetLastError();
                    return fail(FS_ERR_OOM, "body loads: device words");
                }
                FS_HIP(hipMemsetAsync(sh.p, 0, sh.n * sizeof(unsigned long long), st));   // the fold keeps them zero
                words = std::move(w);
                shards = std::move(sh);
            }
            FS_HIP(hipMemsetAsync(words.p, 0, words.n * sizeof(unsigned long long), st));
            for (uint64_t& c : steps) c = 0;
        }
        on = on_;
        return FS_OK;
    }
    // The words of `slot` behind every step enqueued so far, and its step count; reset: zeroed behind the read, on the stream.  Blocking.
    fs_status read(hipStream_t st, uint32_t slot, bool reset, unsigned long long (&w)[WORDS], uint64_t* steps_out) {
        *steps_out = steps[slot];
        hipError_t e = hipMemcpyAsync(w, words.p + slot * WORDS, SLOT_BYTES, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && reset) e = zero(st, slot);
        const hipError_t es = hipStreamSynchronize(st);             // before `w` leaves the caller's scope, whatever happened
        if (e == hipSuccess) e = es;
        return e == hipSuccess ? FS_OK : fail(FS_ERR_DEVICE, hipGetErrorString(e));
    }
};

// Opt-in moving bodies (build extension; single-domain handles): fs_body_* in engine_features.hip.  Per slot a
// field of push vectors over the body's own box and the motion the host last set; w == 0: the slot is free, and never created:
// no allocation, no launch.
struct BodySlot2 {
    DevArray<float2> field;
    uint32_t w = 0, h = 0;
    fs_vec2 extent{};
    fs_body_motion motion{};
    size_t pixels() const { return (size_t)w * h; }
};
struct Bodies : BodySlots<BodySlot2, FS_MAX_BODIES> {
    using Slot = BodySlot2;
    using Loads = BodyLoads<FS_MAX_BODIES, BODY_LOAD_WORDS>;       // five words per body
    Loads loads;
    // This step's pass, behind the force launches, on the state they stored (A.pos_out / A.vel_out; aos: the live 32-B records,
    // or null): the fields and the motions as they are now, by value, the slots in use in ascending order (fs_body_* order their
    // writes and frees on the stream behind it).  `done`: the step's completion event, which this launch carries in the force
    // pass's place.  No slot in use: nothing is launched.  Loads on: the pass's second form and its fold, which carries `done`.
    void enqueue(hipStream_t st, const StepParams& P, const StepArrays& A, void* aos, hipEvent_t done) {
        Bodies2 B;
        BodyLoadMap M{};
        uint32_t c = 0;
        for (uint32_t k = 0; k < FS_MAX_BODIES; ++k) {
            const Slot& b = slot[k];
            if (!b.w) continue;
            const fs_body_motion& m = b.motion;
            M.slot[c] = k;
            Body2& K = B.body[c++];
            K.field = b.field.p; K.w = b.w; K.h = b.h;
            K.ex = b.extent.x; K.ey = b.extent.y;
            K.hx = b.extent.x * 0.5f; K.hy = b.extent.y * 0.5f;
            K.cx = m.centre.x; K.cy = m.centre.y;
            K.r00 = m.rot[0]; K.r01 = m.rot[1]; K.r10 = m.rot[2]; K.r11 = m.rot[3];
            K.ux = m.velocity.x; K.uy = m.velocity.y;
            K.wz = m.angular_velocity;
        }
        if (!c) return;
        for (uint32_t k = c; k < BODIES2_MAX; ++k) B.body[k] = Body2{};
        B.count = M.count = c;
        if (!loads.on) { launch_bodies(st, P, A, B, aos, done); return; }
        launch_bodies_loads(st, P, A, B, aos, M, loads.shards.p, loads.words.p, done);
        for (uint32_t k = 0; k < c; ++k) loads.steps[M.slot[k]] += 1u;
    }
};

// Scratch of a removal (fs_remove_* in engine_count.hip, fs3_remove_* in engine_3d_count.hip), allocated by
// the first one for `capacity` slots and released by fs_reserve / fs3_reserve.  Never called: no allocation, no launch.
struct RemoveScratch {
    DevArray<uint8_t> flags;        // per slot: removed
    DevArray<uint32_t> sums;        // per workgroup of the flags pass: survivors, then offsets; the total behind them
    fs_status reserve(uint32_t capacity) {
        if (flags.p) return FS_OK;
        if (flags.alloc(capacity) == hipSuccess && sums.alloc((size_t)remove_workgroups(capacity) + 1) == hipSuccess) return FS_OK;
        (void)hipGetLastError();
        release();
        return fail(FS_ERR_OOM, "removal: device scratch");
    }
    void release() { flags.release(); sums.release(); }
};

// Scratch of the fluid diagnostics of either handle (fs_stats_* in engine_stats.hip, fs3_stats_* in engine_3d_stats.hip; DESIGN.md
// §29), allocated by the first call and kept for the life of the handle: the partials slab (STATS_MAX_BLOCKS rows, whatever the
// count becomes; nothing in it needs to be zero) and the record the blocking form reads back.  Never called: no allocation, no launch.
struct StatsScratch {
    DevArray<unsigned long long> slab;
    DevArray<unsigned long long> record;
    fs_status reserve(int dims, size_t record_bytes) {
        if (slab.p) return FS_OK;
        if (slab.alloc((size_t)STATS_MAX_BLOCKS * stats_words(dims)) == hipSuccess && record.alloc((record_bytes + 7) / 8) == hipSuccess) return FS_OK;
        (void)hipGetLastError();
        slab.release(); record.release();
        return fail(FS_ERR_OOM, "stats: device scratch");
    }
    // The blocking form behind its checks: `enqueue(out_dev)` puts the two launches on `st`; then one copy of the record and a
    // synchronise.
    template <class Rec, class Enqueue>
    fs_status read(hipStream_t st, Rec* out, Enqueue enqueue) {
        FS_TRY(enqueue((Rec*)record.p));
        FS_HIP(hipMemcpyAsync(out, record.p, sizeof(Rec), hipMemcpyDeviceToHost, st));
        FS_HIP(hipStreamSynchronize(st));
        return FS_OK;
    }
};

// Everything only a slab (multi-GPU) handle has: engine_slab.hip. Torn down like the handle itself, in reverse order of
// declaration: the device arrays, then the events, the exchange stream last.
struct SlabState {
    Stream comm;                    // the exchange's stream (fs_slab_exchange, or the caller's transport between comm_begin / comm_end)
    Event ev_packed;                // main stream: both outgoing messages are complete
    Event ev_exch;                  // comm stream: both incoming messages have arrived
    Event ev_fork2;                 // edge-first: the density pass is done, the edge columns' chain may start on `comm`

    fs_slab_config cfg{};
    uint32_t main_slots = 0;        // capacity - 2 * recv_capacity
    bool counting = true;           // the handle's sort is the counting sort (else the network: serial step only)
    bool packed = false;            // between fs_slab_pack and fs_slab_step
    uint32_t state_lo = 0, state_hi = 0;   // the owned window the current keys / cell starts were built with

    // Overlapped slab step (counting sort only): fs_slab_pack enqueues the pack AND the whole step of the
    // interior columns; the halo exchange runs beside it on `comm`; fs_slab_step finishes the columns within `boundary_cols`
    // of a slab edge on the strip arrays (kernels_strip.hip).
    bool transposed = false;               // cell ids column-major (fs_device.h StepParams::transposed): ranks with neighbours, not the strip step
    bool overlap = false;                  // FS_SLAB_STRIPS: ghosts stay out of the main array, boundary strips after the exchange
    bool edge_first = false;               // the default: the next step's messages are built right after the edge columns' force launch
    PrebuiltMessages pre;                  // edge-first
    uint32_t msg_epoch = 0;                // one number per k_slab_msg launch (its look-back state is never cleared)
    fs_tick_settings last_tick{};
    bool exch_pending = false;             // fs_slab_step must wait for ev_exch
    bool join_pending = false;             // edge-first: the simulation's stream has not yet waited for the edge columns' chain of the last step (slab_join)
    uint32_t boundary_cols = 4;            // owned columns per neighboured edge left to the strips (>= 3)
    uint32_t pending_shift = 0;            // columns a window edge moved since the last pack: that step's migrants land deeper
    // Columns of the overlapped step last planned (plan_overlap).  A strips step is planned by fs_slab_pack and finished from
    // this by fs_slab_step; the next fs_slab_pack of an edge-first handle checks its classification against these interior columns.
    OverlapPlan last_plan;
    bool prof = false;                     // profiling state latched by fs_slab_pack for the matching fs_slab_step

    DevArray<uint2> blockcnt;           // per 256-slot block: records for the left / right message (k_slab_pack)
    DevArray<uint32_t> stage;           // ... and the slots themselves, 2 x 256 entries per block
    DevArray<u64> msg_state;            // k_slab_msg's look-back words
    DevArray<uint32_t> counters;        // [0] n_live, [2] lost, [3] overflow, [4] far_halo
    DevArray<uint32_t> hist;
    // The strip's own particle array (ParticleArrays; its force pass writes pos_out / vel_out, which the write-back scatters
    // into the main array through `back`).
    struct Strip : ParticleArrays {
        DevArray<float2> pos_out, vel_out;
        DevArray<uint32_t> back, rowbase, counters;
        uint32_t cap = 0;
        StepArrays step_arrays() const {
            StepArrays A = ParticleArrays::step_arrays();
            A.pos_out = pos_out.p; A.vel_out = vel_out.p;
            A.n_dev = counters.p + 2;      // strip_counters[2]: slots in use
            return A;
        }
        // what the strip launchers see (fs_kernels.h); ncell_alloc: the handle's allocated cell count
        StripArrays strip_arrays(uint32_t ncell_alloc) const {
            StripArrays T;
            T.cap = cap; T.pos = pos.p; T.vel = vel.p; T.kt = counting_sort_kt(csort.p, cap, ncell_alloc);
            T.hist = counting_sort_hist(csort.p); T.back = back.p; T.rowbase = rowbase.p; T.safe = safe.p; T.counters = counters.p;
            T.pairs = pairs.p; T.pos_out = pos_out.p; T.vel_out = vel_out.p; T.pred = pred.p; T.rho = rho.p;
            return T;
        }
    } strip;

    // where last step's migrants sit: an overlapped (strips) step leaves them in the 2R slots past the main ones
    uint32_t migrant_slots() const { return overlap ? 2u * cfg.recv_capacity : 0u; }
    // one set of messages as the slab launchers see it; a side without a neighbour has no buffer
    SlabMessages messages(const void* left, const void* right, uint32_t epoch = 0) const {
        return {cfg.recv_capacity, (int)cfg.has_left, (int)cfg.has_right, cfg.has_left ? const_cast<void*>(left) : nullptr,
                cfg.has_right ? const_cast<void*>(right) : nullptr, epoch};      // (the unpack launchers only read the buffers)
    }
};

}  // namespace fsd

// Every resource is held by an owner (fs_host.h) and freed by `delete`.  Teardown order: members go in reverse order of
// declaration, then the bases from right to left — so first a slab handle's own state (SlabState: its device arrays, its events,
// its stream), then the device arrays (tracking's, surface tension's, the other members below, then ParticleArrays), then
// HandleQueues backwards: the events (profile ring, sort policy, the named ones), and the streams last.  fs_destroy synchronises
// both streams before any of it.
struct fs_sim : fsd::HandleQueues, fsd::ParticleArrays {
    fs_settings settings{};
    fs_options opts{};
    uint32_t n = 0, capacity = 0;
    uint32_t grid_w = 0, grid_h = 0, ncell = 0;
    uint32_t tick = 0;
    fs_uniform uniform{};
    int device = 0;

    // the main array: ParticleArrays, and
    fsd::DevArray<uint32_t> key;         // keys of an uploaded / initial state; after a step they live in `pairs` (key_in_pairs)
    bool key_in_pairs = false;
    bool rho_in_rho2 = false;       // likewise the densities: rho2.x after a strict / ulp step, `rho` after an upload or a tolerance step
    fsd::DevArray<uint32_t> sort_dirty;  // per-tile flags of the bitonic sort
    fsd::DevArray<float2> tex;           // force field
    bool tex_zero = true;           // the host knows every entry is +-0 (zero-initialised, or an all-zero upload)
    fsd::DevArray<unsigned char> work;   // gap worklist
    uint32_t work_cap = 0;
    fsd::DevArray<fs_particle> aos;      // lazily allocated 32-byte view
    bool aos_live = false;          // a hand-off is registered: the force pass writes the AoS records itself
    uint32_t aos_tick = 0xFFFFFFFFu;   // tick whose state the AoS view holds (only meaningful with aos_live)
    fsd::SurfaceTension st;         // the opt-in features' state: one line each in enqueue_step
    fsd::Tracking trk;
    fsd::Diffusion dif;
    fsd::Bodies bodies;
    fsd::RemoveScratch removal;     // (not a per-step feature: emission and removal happen between steps)
    fsd::StatsScratch stats;        // (nor this: fluid diagnostics are opt-in by being called)
    // what walks the cell table off the step path (engine_query.hip: fs_render_density; field sampling): the records
    // and the cell table belong together — a step has been enqueued since create and since the last fs_upload_particles /
    // fs_upload_start_indices
    bool walk_ready = false;

    fsd::ConstDiv div_2h3{}, div_h2{};   // exact constant divisions of the force pass, proven at create
    fsd::ConstDiv div_h{};               // ... and of the cell coordinates (x / h), over the numerators clamped positions give
    bool rcp_ok = false, sqrt_ok = false; // rcp_rn_fast / sqrt_rn_fast proven on this device at create

    // the main array as the step launchers see it
    fsd::StepArrays step_arrays() const {
        fsd::StepArrays A = ParticleArrays::step_arrays();
        A.tex = tex.p; A.work = work.p; A.key_s = key.p;
        return A;
    }
    // ... and, on a slab handle, as the slab launchers see it
    fsd::SlabArrays slab_arrays() const {
        const fsd::SlabState& S = *slab;
        fsd::SlabArrays A;
        static_cast<fsd::StepArrays&>(A) = step_arrays();
        A.cap = capacity; A.main_slots = S.main_slots; A.counting = S.counting; A.overlap = S.overlap; A.aos = aos.p;
        A.out = S.counting ? fsd::counting_sort_kt(csort.p, capacity, ncell) : pairs.p;
        A.hist = fsd::counting_sort_hist(csort.p);
        A.blockcnt = S.blockcnt.p; A.stage = S.stage.p; A.msg_state = S.msg_state.p; A.counters = S.counters.p;
        return A;
    }
    // the side stream of the force pass and what the sort policy's reports of a few steps ago suggest for its follow-up launches
    fsd::ForceLaunch force_launch() const {
        fsd::ForceLaunch L;
        L.side = side; L.ev_fork = ev_fork; L.ev_join = ev_join;
        L.general_grid = sortp.general_grid(); L.general_hint = sortp.general_hint();
        return L;
    }

    std::unique_ptr<fsd::SlabState> slab;   // slab (multi-GPU) mode; empty on a plain handle
};

namespace fsd {

// ---- engine.hip ---------------------------------------------------------------------------------------------------
// src/simulation.rs:140-141
void grid_dims(const fs_settings& s, uint32_t* gw, uint32_t* gh);
bool settings_valid(const fs_settings& s, std::string* why);
// src/simulation.rs:470-497
void host_uniform(const fs_settings& s, const fs_tick_settings& t, uint32_t tick, fs_uniform* u);
// Step parameters of the handle for the uniform of some tick and, on a slab handle, some owned window [own_lo, own_hi).
StepParams make_params(const fs_sim& s, const fs_uniform& u, uint32_t own_lo = 0, uint32_t own_hi = 0);
// What fs_create_ex and fs_slab_create share, once settings, sort mode, capacity and grid are set (create_common), and what both
// end with after the initial state is in place (create_finish).
fs_status create_common(fs_sim* s);
fs_status create_finish(fs_sim* s);
// After a synchronisation of the stream: a barrier time-out of the sort's stand-by kernel makes the state undefined from
// that step on — whoever is about to receive state (or a "finished" signal) must hear about it (SortPolicy::health).
fs_status sort_health(fs_sim* s);
// The device check of every call that takes an ordinal: `device` names a HIP device of this process, which becomes the current
// one.  No device at all is FS_ERR_DEVICE; an ordinal outside [0, ndev) is FS_ERR_INVALID from the create calls and
// FS_ERR_DEVICE (`out_of_range`) from the calls that work without a handle.
fs_status use_device(int device, fs_status out_of_range = FS_ERR_INVALID);
// Create-time proofs, exhaustive, on the device; blocking.  prove_constdiv: x / c == div_const_fast(x, c, RN(1/c)) for every f32 x
// with 2^-60 <= |x| <= hi (hi == 0: c, the force kernel's numerators); out->ok stays 0 where the proof does not apply, fails, or is not `enabled`.
// prove_rcp_sqrt: the lean reciprocal / square root of the shared-denominator path over their whole ranges (both false under
// FS_NO_SHAREDIV).  The scratch words are device memory the proof may overwrite.
fs_status prove_constdiv(hipStream_t st, uint32_t* scratch_word, float c, ConstDiv* out, float hi = 0.0f, bool enabled = true);
fs_status prove_rcp_sqrt(hipStream_t st, uint32_t* scratch_two_words, bool* rcp_ok, bool* sqrt_ok);

// ---- engine_slab.hip: what a plain entry point asks of a slab handle (no-ops on a plain one) -----------------
// Edge-first slab step: the edge columns' chain of the last step (exchange stream) has advanced its particles and classified their
// slots; the simulation's stream only waits for it when something other than the next pack -> exchange -> step cycle needs that
// state (the cycle itself is ordered by the exchange's event).  Every entry point that reads or replaces the state calls this.
fs_status slab_join(fs_sim* s);
#define FS_JOIN(s) FS_TRY(fsd::slab_join(s))
fs_status slab_sync(fs_sim* s);    // fs_sync: an exchange or edge chain still in flight on the exchange stream

}  // namespace fsd
