// engine_slab.hip — host side of the multi-GPU "slab" handles of the C ABI (include/fluidsim.h, fs_slab_*): one rank's window
// of columns, the pack -> exchange -> step cycle in its three step modes (serial, edge-first, strips), and what
// re-balancing reads.  The handle itself and the plain step: engine.hip; the opt-in features, none of which a slab handle
// has: engine_features.hip, engine_query.hip.  Everything slab-only a handle holds: SlabState (engine.h).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "engine.h"

using namespace fsd;

namespace {

// workgroups of the edge columns' launches in an edge-first step with column-major ids (each walks the device-side block ranges)
#define FS_EDGE_GRID 1024u

// Step parameters of the current tick and the owned window as configured.
StepParams slab_params(const fs_sim& s) { return make_params(s, s.uniform, s.slab->cfg.own_lo, s.slab->cfg.own_hi); }

// Stored keys, cell starts and the column origin belong to the window of the LAST step (or import); a
// window set since then (fs_slab_set_window) only takes effect at the next pack.  Anything that reads
// the stored state back in global coordinates must use this.
StepParams params_of_state(const fs_sim& s) {
    const SlabState& S = *s.slab;
    return S.state_hi > S.state_lo ? make_params(s, s.uniform, S.state_lo, S.state_hi) : slab_params(s);
}

// ---- overlapped slab step --------------------------------------------------------------------------
// Step parameters of the two force launches of an overlapped step: the interior launch (main array) and the strip launch.
StepParams overlap_params(const fs_sim& s, const OverlapPlan& plan, bool strip) {
    const SlabState::Strip& T = s.slab->strip;
    StepParams P = slab_params(s);
    P.adv_lo = plan.adv_lo; P.adv_hi = plan.adv_hi;
    P.adv_outside = strip ? 1 : 0;
    if (strip) { P.n = T.cap; P.n_live = T.counters.p; if (P.block_bounds) P.block_bounds = T.bbounds.p; }
    return P;
}

// Interior columns and strip windows of a step whose boundary zone is `z` columns deep.  Local columns: 0 and W-1 are padding,
// 1..2 and W-3..W-2 the ghost columns, own_lo is local column 3 (make_params).
OverlapPlan plan_overlap(const fs_slab_config& c, uint32_t z) {
    OverlapPlan p;
    const uint32_t width = c.own_hi - c.own_lo, W = width + 6u;
    const uint32_t zl = c.has_left ? z : 0u, zr = c.has_right ? z : 0u;
    p.strip_active = c.has_left || c.has_right;
    if (zl + zr >= width) {                        // no interior: the strip holds the whole window
        p.adv_lo = p.adv_hi = c.own_lo;
        if (p.strip_active) { p.win[0] = 1u; p.win[1] = W - 1u; }
        return p;
    }
    p.adv_lo = c.own_lo + zl; p.adv_hi = c.own_hi - zr;
    // a window = the two ghost columns + the boundary columns + two columns of interior context
    const uint32_t lhi = 3u + zl + 2u, rlo = (W - 3u) - zr - 2u;
    if (c.has_left && c.has_right && lhi >= rlo) { p.win[0] = 1u; p.win[1] = W - 1u; return p; }
    if (c.has_left) { p.win[0] = 1u; p.win[1] = lhi < W - 1u ? lhi : W - 1u; }
    if (c.has_right) { p.win[2] = rlo > 1u ? rlo : 1u; p.win[3] = W - 1u; }
    return p;
}
// ... of the step being enqueued: the configured boundary zone, widened once by the columns a window edge has moved
OverlapPlan plan_step(SlabState& S) { return S.last_plan = plan_overlap(S.cfg, S.boundary_cols + std::exchange(S.pending_shift, 0u)); }

// Second half of fs_slab_pack of a strips handle: everything that does not need the incoming messages.
fs_status slab_interior(fs_sim* s) {
    SlabState& S = *s->slab;
    hipStream_t st = s->stream;
    FS_HIP(hipEventRecord(S.ev_packed, st));       // the outgoing messages are complete: the exchange may start
    const OverlapPlan plan = plan_step(S);
    const StepParams P = overlap_params(*s, plan, false);
    hipEvent_t* ev = S.prof ? s->prof.current() : nullptr;
    if (ev) FS_HIP(hipEventRecord(ev[1], st));
    launch_counting_sort_pairs(st, s->capacity, P.ncell, s->ncell, s->cs.p, s->csort.p, S.counters.p, s->tick, nullptr, s->safe.p);
    if (ev) FS_HIP(hipEventRecord(ev[2], st));
    const SlabArrays A = s->slab_arrays();
    launch_counting_reorder_slab(st, P, A, s->capacity, s->ncell);
    if (plan.strip_active)                          // the main array's share of the strips: also independent of the messages
        launch_strip_gather(st, P, A, S.strip.strip_arrays(s->ncell), plan, S.cfg.recv_capacity);
    if (ev) FS_HIP(hipEventRecord(ev[3], st));
    launch_density(st, P, A);
    if (ev) FS_HIP(hipEventRecord(ev[4], st));
    launch_force(st, P, A, s->force_launch());
    if (ev) FS_HIP(hipEventRecord(ev[5], st));
    FS_HIP(hipGetLastError());
    return FS_OK;
}

// fs_slab_step of a strips handle: the boundary strips, after the incoming messages.
fs_status step_strips(fs_sim* s, const void* recv_left, const void* recv_right) {
    SlabState& S = *s->slab;
    hipStream_t st = s->stream;
    if (S.exch_pending) { FS_HIP(hipStreamWaitEvent(st, S.ev_exch, 0)); S.exch_pending = false; }
    hipEvent_t* ev = S.prof ? s->prof.current() : nullptr;
    const OverlapPlan& plan = S.last_plan;          // fs_slab_pack's (slab_interior)
    if (plan.strip_active) {
        SlabState::Strip& T = S.strip;
        const StepParams P = overlap_params(*s, plan, false), PS = overlap_params(*s, plan, true);
        const SlabArrays SA = s->slab_arrays();
        const StripArrays TS = T.strip_arrays(s->ncell);
        launch_strip_unpack(st, P, SA, TS, S.messages(recv_left, recv_right));
        launch_counting_sort_pairs(st, T.cap, PS.ncell, s->ncell, T.cs.p, T.csort.p, T.counters.p, s->tick, T.counters.p + 2);
        StepArrays TA = T.step_arrays();
        TA.tex = s->tex.p;
        launch_counting_reorder_slab(st, PS, TA, T.cap, s->ncell);
        launch_density(st, PS, TA);
        ForceLaunch L;
        L.general_grid = 256u;
        launch_force(st, PS, TA, L);
        launch_strip_writeback(st, PS, SA, TS);
    }
    if (ev) { FS_HIP(hipEventRecord(ev[6], st)); s->prof.pending += 1; }
    FS_HIP(hipGetLastError());
    S.packed = false;
    return FS_OK;
}

// fs_slab_step behind the reorder pass, serial step: one density and one force launch over every owned column.
fs_status step_serial(fs_sim* s, const StepParams& P, const StepArrays& A, hipEvent_t* ev) {
    hipStream_t st = s->stream;
    launch_density(st, P, A);
    if (ev) FS_HIP(hipEventRecord(ev[4], st));
    ForceLaunch LI = s->force_launch();
    LI.quad_entries = s->sortp.quad_entries();
    launch_force(st, P, A, LI);
    if (ev) { FS_HIP(hipEventRecord(ev[5], st)); FS_HIP(hipEventRecord(ev[6], st)); s->prof.pending += 1; }
    return FS_OK;
}

// ... edge-first step.  Behind the density pass the stream forks: the handle's exchange stream (high priority) advances
// the owned columns within boundary_cols of a neighboured edge — a few hundred blocks, latency-bound — then builds the
// NEXT step's messages from their new state (k_slab_prepack .. k_slab_gather) and carries the exchange of those
// messages (fs_slab_exchange / the caller's transport between fs_slab_comm_begin / _end); the simulation's stream
// runs the force pass of the interior columns beside all that, and joins before anything reads the new state.
// `forked`: the reorder kernel has signalled ev_fork2 (column-major ids, a non-empty interior).
fs_status step_edge_first(fs_sim* s, const StepParams& P, const SlabArrays& A, const OverlapPlan& plan, bool forked, hipEvent_t* ev) {
    SlabState& S = *s->slab;
    hipStream_t st = s->stream, es = S.comm;
    if (forked) {
        // column-major ids: the edge columns' chain forks off BEFORE the density pass — their own density launch (the few
        // hundred blocks that hold the edge columns and one column more on either side; the full launch below computes the
        // same values again) runs on the exchange stream, so the chain is done, and the exchange under way, early in the
        // interior columns' force pass
        StepParams PD = P;
        PD.adv_lo = plan.adv_lo; PD.adv_hi = plan.adv_hi;
        FS_HIP(hipStreamWaitEvent(es, S.ev_fork2, 0));           // signalled by the reorder kernel itself
        launch_density(es, PD, A, FS_EDGE_GRID);
    }
    launch_density(st, P, A);
    if (ev) FS_HIP(hipEventRecord(ev[4], st));
    ForceLaunch LI = s->force_launch();          // the launch on the simulation's stream: the interior columns
    LI.quad_entries = s->sortp.quad_entries();
    StepParams PE = P, PI = P;
    PE.adv_lo = PI.adv_lo = plan.adv_lo; PE.adv_hi = PI.adv_hi = plan.adv_hi;
    PE.adv_outside = 1; PI.adv_outside = 0;
    // column-major ids: the edge columns are a few hundred consecutive blocks at the two ends of the sorted array, walked by
    // small fixed grids (fs_device.h EdgeBlocks)
    const uint32_t eg = S.transposed ? FS_EDGE_GRID : 0u;
    if (!forked) FS_HIP(hipEventRecord(S.ev_fork2, st));
    // the simulation's stream first (its force launch is the long one: the host must not leave that stream empty while it
    // enqueues the six launches of the edge chain — seen under the profiler, where a launch costs 10 us), then the chain
    if (plan.adv_lo < plan.adv_hi) launch_force(st, PI, A, LI);
    if (ev) FS_HIP(hipEventRecord(ev[5], st));      // FS_PASS_FORCE: the interior launch
    if (!forked) FS_HIP(hipStreamWaitEvent(es, S.ev_fork2, 0));
    ForceLaunch LE;                      // the chain's own launches: one stream, a small general grid
    LE.general_grid = 256u; LE.edge_grid = eg;
    launch_force(es, PE, A, LE);
    {   // what fs_slab_pack will see at tick + 1, if nothing changes in between (it checks)
        fs_uniform un;
        host_uniform(s->settings, S.last_tick, s->tick + 1, &un);
        StepParams PN = make_params(*s, un, S.cfg.own_lo, S.cfg.own_hi);
        PN.adv_lo = plan.adv_lo; PN.adv_hi = plan.adv_hi; PN.adv_outside = 1;
        launch_slab_prepack(es, PN, A, S.messages(S.pre.left, S.pre.right, ++S.msg_epoch), eg, true);
        S.pre.classified = true;
        FS_HIP(hipEventRecord(S.ev_packed, es));        // the next step's messages are complete (and the edge columns advanced)
        S.pre.built(S.cfg, S.last_tick.delta);
    }
    // no join here: the next fs_slab_pack leaves the edge columns' slots alone, and fs_slab_step waits for the exchange that
    // follows their chain on the exchange stream; anything else that touches the state joins first (slab_join)
    S.join_pending = true;
    if (ev) { FS_HIP(hipEventRecord(ev[6], st)); s->prof.pending += 1; }     // FS_PASS_BOUNDARY: nothing left on this stream
    return FS_OK;
}

}  // namespace

fs_status fsd::slab_join(fs_sim* s) {
    if (s && s->slab && s->slab->join_pending) {
        FS_HIP(hipStreamWaitEvent(s->stream, s->slab->ev_packed, 0));
        s->slab->join_pending = false;
    }
    return FS_OK;
}

fs_status fsd::slab_sync(fs_sim* s) {
    if (!s->slab) return FS_OK;
    SlabState& S = *s->slab;
    // an exchange issued but not yet consumed by fs_slab_step / the edge columns' chain of the last edge-first step
    if (S.comm && (S.exch_pending || S.join_pending)) { FS_HIP(hipStreamSynchronize(S.comm)); S.join_pending = false; }
    return FS_OK;
}

extern "C" {

fs_status fs_slab_create(const fs_settings* settings, int device, const fs_slab_config* cfg, fs_sim** out) {
    if (!settings || !cfg || !out) return fail(FS_ERR_INVALID, "null argument");
    *out = nullptr;
    std::string why;
    if (!settings_valid(*settings, &why)) return fail(FS_ERR_INVALID, why);
    uint32_t gw, gh;
    grid_dims(*settings, &gw, &gh);
    if (cfg->own_lo >= cfg->own_hi || cfg->own_hi > gw) return fail(FS_ERR_INVALID, "bad owned window");
    if (cfg->own_hi - cfg->own_lo < 4) return fail(FS_ERR_INVALID, "slab narrower than 4 columns");
    if (cfg->max_cols < cfg->own_hi - cfg->own_lo) return fail(FS_ERR_INVALID, "max_cols < window");
    if (cfg->capacity <= 2 * cfg->recv_capacity || cfg->recv_capacity == 0)
        return fail(FS_ERR_INVALID, "capacity must exceed 2*recv_capacity");
    if (cfg->capacity > (1u << 28)) return fail(FS_ERR_INVALID, "capacity > 2^28");
    if (cfg->recv_capacity >= (1u << 20) - 2u) return fail(FS_ERR_INVALID, "recv_capacity >= 2^20 - 2 (message counters are 20-bit fields)");
    FS_TRY(use_device(device));

    std::unique_ptr<fs_sim> s(new (std::nothrow) fs_sim());     // an error exit frees whatever the handle holds by then
    if (s) s->slab.reset(new (std::nothrow) SlabState());
    if (!s || !s->slab) return fail(FS_ERR_OOM, "host allocation failed");
    SlabState& S = *s->slab;
    s->settings = *settings;
    fs_options_default(&s->opts);
    s->opts.device = device;
    s->opts.ref_quirks = 0;
    // per-rank sorts can only be tolerance-parity with a single-domain run, so slabs
    // default to the O(N) counting sort; cfg->sort_mode = 1 + FS_SORT_BITONIC selects the network
    s->opts.sort_mode = (cfg->sort_mode & 0xFFu) == 1 + FS_SORT_BITONIC ? FS_SORT_BITONIC : FS_SORT_COUNTING;
    S.counting = s->opts.sort_mode == FS_SORT_COUNTING;
    {   // the overlapped step needs the counting sort (ghosts out of the main array); FS_SLAB_SERIAL / FS_SLAB_OVERLAP=0: the serial step
        // FS_SLAB_MODE=serial|edge|strips overrides the configuration (A/B runs)
        const char* e = getenv("FS_SLAB_MODE");
        uint32_t m = (cfg->sort_mode & FS_SLAB_SERIAL) ? 0u : (cfg->sort_mode & FS_SLAB_STRIPS) ? 2u : 1u;
        if (e) m = !strcmp(e, "serial") ? 0u : !strcmp(e, "strips") ? 2u : !strcmp(e, "edge") ? 1u : m;
        if (!S.counting) m = 0u;               // the network's slab mode stays the serial step (bit-identity with the plain engine)
        S.overlap = m == 2u;
        S.edge_first = m == 1u;
        // column-major cell ids wherever a slab edge has a neighbour (the edge columns are then whole blocks at the two ends of the
        // sorted array); a slab without neighbours keeps the reference layout and stays bit-identical to the plain engine in
        // FS_SORT_COUNTING mode.  FS_SLAB_TRANSPOSE=0/1 overrides (A/B runs); the strip step's gather is written for rows.
        const char* te = getenv("FS_SLAB_TRANSPOSE");
        S.transposed = S.counting && !S.overlap && (cfg->has_left || cfg->has_right) && !(cfg->sort_mode & FS_SLAB_ROWMAJOR);
        if (te && S.counting && !S.overlap) S.transposed = atoi(te) != 0;
    }
    s->device = device;
    S.cfg = *cfg;
    s->capacity = cfg->capacity;
    s->n = 0;
    S.main_slots = cfg->capacity - 2 * cfg->recv_capacity;
    s->grid_w = gw; s->grid_h = gh;
    const uint32_t wmax = cfg->max_cols + 6u;
    s->ncell = wmax * gh;                       // allocation size of the local grid
    s->work_cap = s->ncell / 16u + 1024u;
    FS_TRY(create_common(s.get()));
    const size_t cap = s->capacity;
    FS_HIP(s->owned.alloc(cap));
    const size_t nblocks = (cap + 255) / 256;
    FS_HIP(S.blockcnt.alloc(2 * (nblocks + 1)));       // per 256-slot block: message counts, then message offsets (k_slab_msg)
    FS_HIP(S.stage.alloc(slab_stage_words((uint32_t)cap)));
    FS_HIP(S.msg_state.alloc(slab_msg_groups((uint32_t)cap) + 1));
    FS_HIP(hipMemsetAsync(S.msg_state.p, 0, S.msg_state.n * sizeof(u64), s->stream));
    FS_HIP(S.counters.alloc(16));
    FS_HIP(S.hist.alloc(gw));
    if (S.overlap || S.edge_first) {
        int lo_prio = 0, hi_prio = 0;          // the exchange's kernel should not queue behind the interior columns' workgroups
        (void)hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio);
        FS_HIP(hipStreamCreateWithPriority(&S.comm.h, hipStreamNonBlocking, hi_prio));
        FS_HIP(hipEventCreateWithFlags(&S.ev_packed.h, hipEventDisableTiming));
        FS_HIP(hipEventCreateWithFlags(&S.ev_exch.h, hipEventDisableTiming));
        // waited for by the exchange stream of this same device only: no system-scope fence (a write-back of every L2 behind the
        // reorder kernel, which the simulation's own stream would sit out)
        FS_HIP(hipEventCreateWithFlags(&S.ev_fork2.h, hipEventDisableTiming | hipEventDisableSystemFence));
        if (const char* e = getenv("FS_SLAB_BOUNDARY_COLS")) S.boundary_cols = (uint32_t)atoi(e) < 3u ? 3u : (uint32_t)atoi(e);
    }
    if (S.overlap) {
        // The strip could hold every particle of a narrow slab (all columns within the boundary zone) plus both messages:
        // same capacity as the main array (memory is not the constraint: ~100 B per slot); its kernels cover the slots in use only.
        SlabState::Strip& T = S.strip;
        T.cap = (uint32_t)cap;
        FS_HIP(T.alloc_common(cap)); FS_HIP(T.pos_out.alloc(cap)); FS_HIP(T.vel_out.alloc(cap)); FS_HIP(T.owned.alloc(cap));
        FS_HIP(T.csort.alloc(counting_sort_scratch_words((uint32_t)cap, s->ncell)));
        FS_HIP(hipMemsetAsync(T.csort.p, 0, T.csort.n * sizeof(uint32_t), s->stream));
        FS_HIP(T.cs.alloc((size_t)s->ncell + 1)); FS_HIP(T.start_ref.alloc(s->ncell));
        FS_HIP(T.counters.alloc(8)); FS_HIP(T.back.alloc(cap)); FS_HIP(T.rowbase.alloc(2 * (size_t)gh + 2));
        FS_HIP(hipMemsetAsync(T.cs.p, 0, T.cs.n * sizeof(uint32_t), s->stream));
        FS_HIP(hipMemsetAsync(T.counter.p, 0, 8 * sizeof(uint32_t), s->stream));
        FS_HIP(hipMemsetAsync(T.counters.p, 0, 8 * sizeof(uint32_t), s->stream));
        FS_HIP(hipMemsetAsync(T.pred.p, 0, (cap + FS_PRED_SLACK) * sizeof(float2), s->stream));
        FS_HIP(hipMemsetAsync(T.pairs.p, 0xFF, cap * sizeof(u64), s->stream));
    }
    FS_HIP(hipMemsetAsync(S.counters.p, 0, 16 * sizeof(uint32_t), s->stream));
    FS_HIP(hipMemsetAsync(s->owned.p, 0, cap, s->stream));
    FS_HIP(hipMemsetAsync(s->pos.p, 0, cap * sizeof(float2), s->stream));
    FS_HIP(hipMemsetAsync(s->vel.p, 0, cap * sizeof(float2), s->stream));
    FS_HIP(hipMemsetAsync(s->pred.p, 0, cap * sizeof(float2), s->stream));
    FS_HIP(hipMemsetAsync(s->key.p, 0xFF, cap * sizeof(uint32_t), s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    FS_TRY(create_finish(s.get()));
    *out = s.release();
    return FS_OK;
}

fs_status fs_slab_upload_owned(fs_sim* s, const fs_particle* src, size_t n) {
    if (!s || !s->slab || (!src && n)) return fail(FS_ERR_INVALID, "bad argument");
    SlabState& S = *s->slab;
    if (n > S.main_slots) return fail(FS_ERR_INVALID, "more owned particles than main slots");
    FS_JOIN(s);
    S.pre.invalidate();                    // the state is replaced: messages built from the old one are void
    FS_HIP(hipSetDevice(s->device));
    if (n) FS_HIP(hipMemcpyAsync(s->aos.p, src, n * sizeof(fs_particle), hipMemcpyHostToDevice, s->stream));
    launch_slab_import(s->stream, slab_params(*s), s->slab_arrays(), (uint32_t)n);
    const uint32_t nl = (uint32_t)n;
    FS_HIP(hipMemcpyAsync(S.counters.p, &nl, sizeof nl, hipMemcpyHostToDevice, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    S.state_lo = S.cfg.own_lo; S.state_hi = S.cfg.own_hi;
    return FS_OK;
}

fs_status fs_slab_set_window(fs_sim* s, uint32_t own_lo, uint32_t own_hi) {
    if (!s || !s->slab) return fail(FS_ERR_INVALID, "not a slab handle");
    SlabState& S = *s->slab;
    FS_JOIN(s);
    if (own_lo >= own_hi || own_hi > s->grid_w || own_hi - own_lo < 4 || own_hi - own_lo > S.cfg.max_cols)
        return fail(FS_ERR_INVALID, "bad owned window");
    if (S.packed) return fail(FS_ERR_INVALID, "window change between pack and step");
    {   // the particles of a column that changes hands arrive at the new owner as migrants, that many columns deeper than usual:
        // the next (overlapped) step widens its boundary zone by the shift
        const uint32_t dl = S.cfg.has_left ? (own_lo > S.cfg.own_lo ? own_lo - S.cfg.own_lo : S.cfg.own_lo - own_lo) : 0u;
        const uint32_t dr = S.cfg.has_right ? (own_hi > S.cfg.own_hi ? own_hi - S.cfg.own_hi : S.cfg.own_hi - own_hi) : 0u;
        const uint32_t d = dl > dr ? dl : dr;
        if (d > S.pending_shift) S.pending_shift = d;
    }
    S.cfg.own_lo = own_lo;
    S.cfg.own_hi = own_hi;
    return FS_OK;
}

/* Overlapped step: owned columns per neighboured slab edge that are left to the boundary strips (computed AFTER the halo
 * exchange; everything farther inside runs while the messages are in flight).  A migrant must land at least 3 columns short of
 * the interior — cols >= 3 + the columns the fastest particle crosses in one step; violations are counted in far_halo. */
fs_status fs_slab_set_boundary_cols(fs_sim* s, uint32_t cols) {
    if (!s || !s->slab) return fail(FS_ERR_INVALID, "not a slab handle");
    if (s->slab->packed) return fail(FS_ERR_INVALID, "boundary change between pack and step");
    s->slab->boundary_cols = cols < 3u ? 3u : cols;
    return FS_OK;
}
uint32_t fs_slab_boundary_cols(const fs_sim* s) { return (s && s->slab && (s->slab->overlap || s->slab->edge_first)) ? s->slab->boundary_cols : 0u; }
int fs_slab_overlapped(const fs_sim* s) { return (s && s->slab) ? (s->slab->edge_first ? 1 : s->slab->overlap ? 2 : 0) : 0; }
void* fs_slab_comm_stream(const fs_sim* s) { return (s && s->slab) ? (void*)s->slab->comm : nullptr; }

/* Transport hooks of the overlapped step (a no-op on a serial handle, whose exchange is ordered by the simulation's stream):
 * fs_slab_comm_begin makes the exchange stream wait for the packed messages, the caller then issues its send/recv ON
 * fs_slab_comm_stream(), fs_slab_comm_end records their completion for fs_slab_step to wait on.  fs_slab_exchange does all
 * three itself.  fs_slab_wait_packed blocks the HOST until the outgoing messages are complete (host-staged transports). */
fs_status fs_slab_comm_begin(fs_sim* s) {
    if (!s || !s->slab) return fail(FS_ERR_INVALID, "not a slab handle");
    SlabState& S = *s->slab;
    if (!S.comm) return FS_OK;
    FS_HIP(hipSetDevice(s->device));
    if (!S.packed) FS_HIP(hipEventRecord(S.ev_packed, s->stream));   // outside a step: behind whatever the simulation's stream holds
    FS_HIP(hipStreamWaitEvent(S.comm, S.ev_packed, 0));
    return FS_OK;
}
fs_status fs_slab_comm_end(fs_sim* s) {
    if (!s || !s->slab) return fail(FS_ERR_INVALID, "not a slab handle");
    SlabState& S = *s->slab;
    if (!S.comm) return FS_OK;
    FS_HIP(hipSetDevice(s->device));
    FS_HIP(hipEventRecord(S.ev_exch, S.comm));
    S.exch_pending = true;
    return FS_OK;
}
fs_status fs_slab_wait_packed(fs_sim* s) {
    if (!s || !s->slab) return fail(FS_ERR_INVALID, "not a slab handle");
    FS_HIP(hipSetDevice(s->device));
    if (s->slab->comm && s->slab->packed) FS_HIP(hipEventSynchronize(s->slab->ev_packed));
    else FS_HIP(hipStreamSynchronize(s->stream));
    return FS_OK;
}

size_t fs_slab_message_bytes(const fs_sim* s) {
    return (s && s->slab) ? slab_message_bytes(s->slab->cfg.recv_capacity) : 0;
}

fs_status fs_slab_pack(fs_sim* s, const fs_tick_settings* t, void* send_left, void* send_right) {
    if (!s || !s->slab || !t) return fail(FS_ERR_INVALID, "bad argument");
    SlabState& S = *s->slab;
    if (S.packed) return fail(FS_ERR_INVALID, "fs_slab_pack called twice without fs_slab_step");
    if ((S.cfg.has_left && !send_left) || (S.cfg.has_right && !send_right))
        return fail(FS_ERR_INVALID, "missing outgoing message buffer");
    FS_HIP(hipSetDevice(s->device));
    s->tick += 1;
    host_uniform(s->settings, *t, s->tick, &s->uniform);
    const StepParams P = slab_params(*s);
    S.prof = s->prof.on;                   // a toggle between pack and step must not leave ev[0] unrecorded
    if (S.prof) {
        FS_TRY(s->prof.begin());
        FS_HIP(hipEventRecord(s->prof.current()[0], s->stream));
    }
    const SlabArrays A = s->slab_arrays();
    // edge-first step: are the messages of this tick already in the send buffers (built by the last fs_slab_step)?  Only if
    // nothing they depend on has changed since: buffers, owned window, delta.
    const bool pre = S.pre.matches(S.cfg, send_left, send_right, t->delta);
    S.pre.invalidate();
    SlabPack O;
    O.lists = !pre;
    O.prev_adv_lo = S.last_plan.adv_lo; O.prev_adv_hi = S.last_plan.adv_hi;
    // pre: this launch needs nothing of the edge columns' chain (their slots are classified already: skip_edge) — no join; the
    // chain is waited for through the exchange's event in fs_slab_step.  Otherwise: join, and take back the histogram counts
    // that chain added with the parameters it expected (the scan has left the table zero everywhere else)
    O.skip_edge = pre && S.pre.classified;
    if (!pre) {
        FS_JOIN(s);
        if (S.pre.classified && S.counting) FS_HIP(hipMemsetAsync(A.hist, 0, (size_t)s->ncell * sizeof(uint32_t), s->stream));
    }
    S.pre.classified = false;
    const SlabMessages M = S.messages(send_left, send_right, ++S.msg_epoch);
    S.pre.left = M.left; S.pre.right = M.right;
    S.last_tick = *t;
    launch_slab_pack(s->stream, P, A, M, O);
    FS_HIP(hipGetLastError());
    S.packed = true;
    S.state_lo = S.cfg.own_lo; S.state_hi = S.cfg.own_hi;
    if (S.overlap) return slab_interior(s);
    // edge-first: a pre-built message set was recorded complete (ev_packed) when it was built; a fresh one is complete now
    if (S.edge_first && !pre) FS_HIP(hipEventRecord(S.ev_packed, s->stream));
    return FS_OK;
}

// The common front of the serial and the edge-first step (wait for the exchange or join, unpack, sort, reorder), then the
// mode's own density and force launches; a strips handle has its own second half.
fs_status fs_slab_step(fs_sim* s, const void* recv_left, const void* recv_right) {
    if (!s || !s->slab) return fail(FS_ERR_INVALID, "not a slab handle");
    SlabState& S = *s->slab;
    if (!S.packed) return fail(FS_ERR_INVALID, "fs_slab_step without fs_slab_pack");
    if ((S.cfg.has_left && !recv_left) || (S.cfg.has_right && !recv_right))
        return fail(FS_ERR_INVALID, "missing incoming message buffer");
    FS_HIP(hipSetDevice(s->device));
    if (S.overlap) return step_strips(s, recv_left, recv_right);
    const StepParams P = slab_params(*s);
    hipStream_t st = s->stream;
    hipEvent_t* ev = S.prof ? s->prof.current() : nullptr;
    // the exchange was enqueued on the exchange stream behind the edge columns' chain: its event stands for the join as well
    if (S.exch_pending) { FS_HIP(hipStreamWaitEvent(st, S.ev_exch, 0)); S.exch_pending = false; S.join_pending = false; }
    else FS_JOIN(s);
    const SlabArrays A = s->slab_arrays();
    launch_slab_unpack(st, P, A, S.messages(recv_left, recv_right));
    if (ev) FS_HIP(hipEventRecord(ev[1], st));
    if (S.counting) {
        launch_counting_sort_pairs(st, s->capacity, P.ncell, s->ncell, s->cs.p, s->csort.p, S.counters.p, s->tick, nullptr, s->safe.p);
    } else {
        SortPlan per_stage;                    // ghosts arrive at the end of the array every step: they travel far, no shifted merge
        per_stage.fuse_stage = 0;
        launch_bitonic_sort(st, s->pairs.p, s->capacity, s->sort_dirty.p, nullptr, &per_stage);
    }
    if (ev) FS_HIP(hipEventRecord(ev[2], st));
    const bool edge_step = S.edge_first && (S.cfg.has_left || S.cfg.has_right);
    const OverlapPlan plan = edge_step ? plan_step(S) : OverlapPlan();
    const bool forked = edge_step && S.transposed && plan.adv_lo < plan.adv_hi;   // the edge columns' chain forks off behind the reorder pass
    if (S.counting)
        launch_counting_reorder_slab(st, P, A, s->capacity, s->ncell, forked ? S.ev_fork2.h : nullptr);
    else
        launch_slab_reorder(st, P, A, s->work_cap);
    if (ev) FS_HIP(hipEventRecord(ev[3], st));
    FS_TRY(edge_step ? step_edge_first(s, P, A, plan, forked, ev) : step_serial(s, P, A, ev));
    FS_HIP(hipGetLastError());
    S.packed = false;
    return FS_OK;
}

fs_status fs_slab_counters_read(fs_sim* s, fs_slab_counters* out) {
    if (!s || !s->slab || !out) return fail(FS_ERR_INVALID, "bad argument");
    FS_JOIN(s);
    FS_HIP(hipSetDevice(s->device));
    uint32_t c[8];
    FS_HIP(hipMemcpyAsync(c, s->slab->counters.p, sizeof c, hipMemcpyDeviceToHost, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    out->n_live = c[0]; out->lost = c[2]; out->overflow = c[3]; out->far_halo = c[4];
    return FS_OK;
}

fs_status fs_slab_max_speed(fs_sim* s, float* out) {
    if (!s || !s->slab || !out) return fail(FS_ERR_INVALID, "bad argument");
    SlabState& S = *s->slab;
    if (S.packed) return fail(FS_ERR_INVALID, "fs_slab_max_speed between pack and step");
    FS_JOIN(s);
    FS_HIP(hipSetDevice(s->device));
    uint32_t bits = 0;
    FS_HIP(hipMemsetAsync(S.counters.p + 5, 0, sizeof(uint32_t), s->stream));
    launch_slab_maxspeed(s->stream, s->slab_arrays(), S.migrant_slots());
    FS_HIP(hipMemcpyAsync(&bits, S.counters.p + 5, sizeof bits, hipMemcpyDeviceToHost, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    std::memcpy(out, &bits, sizeof bits);
    return FS_OK;
}

/* Re-balancing inputs left ON THE DEVICE, on the simulation's stream, nothing read back: `hist_dev[grid_w_global]` =
 * particles per global column (zero outside the owned window), `stats_dev[4]` = {lost, overflow, far_halo, bits of the
 * largest owned |velocity|} — all four reduce with MAX as u32 (non-negative floats order like their bits).  The caller
 * all-reduces both buffers (fs_comm_allreduce, or any collective ordered after this stream) and reads them once. */
fs_status fs_slab_rebalance_stats(fs_sim* s, uint32_t* stats_dev, uint32_t* hist_dev, size_t grid_w_global) {
    if (!s || !s->slab || !stats_dev || !hist_dev || grid_w_global < s->grid_w) return fail(FS_ERR_INVALID, "bad argument");
    SlabState& S = *s->slab;
    if (S.packed) return fail(FS_ERR_INVALID, "fs_slab_rebalance_stats between pack and step");
    FS_JOIN(s);
    FS_HIP(hipSetDevice(s->device));
    const StepParams P = params_of_state(*s);
    const SlabArrays A = s->slab_arrays();
    FS_HIP(hipMemsetAsync(hist_dev, 0, grid_w_global * sizeof(uint32_t), s->stream));
    launch_slab_colhist(s->stream, P, A, hist_dev, S.migrant_slots());
    FS_HIP(hipMemsetAsync(S.counters.p + 5, 0, sizeof(uint32_t), s->stream));
    launch_slab_maxspeed(s->stream, A, S.migrant_slots());
    // counters [2] lost, [3] overflow, [4] far_halo, [5] max-speed bits are adjacent
    FS_HIP(hipMemcpyAsync(stats_dev, S.counters.p + 2, 4 * sizeof(uint32_t), hipMemcpyDeviceToDevice, s->stream));
    FS_HIP(hipGetLastError());
    return FS_OK;
}

fs_status fs_slab_download(fs_sim* s, fs_particle* dst, uint8_t* owned, size_t cap, uint32_t* n_live) {
    if (!s || !s->slab || !dst || !owned || !n_live) return fail(FS_ERR_INVALID, "bad argument");
    SlabState& S = *s->slab;
    FS_JOIN(s);
    FS_HIP(hipSetDevice(s->device));
    const StepParams P = params_of_state(*s);
    uint32_t nl = 0;
    FS_HIP(hipMemcpyAsync(&nl, S.counters.p, sizeof nl, hipMemcpyDeviceToHost, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    if (nl > s->capacity) nl = s->capacity;
    // overlapped step: the sorted prefix [0, nl) (owned + this rank's near-leavers) and, past the main slots, the 2R slots
    // that mirror the incoming messages — the migrants among them carry the owned flag; returned back to back
    const size_t migr = S.migrant_slots();
    if (S.overlap && nl > S.main_slots) nl = S.main_slots;
    const size_t n = nl < cap ? nl : cap;
    const size_t m = cap - n < migr ? cap - n : migr;
    *n_live = (uint32_t)(n + m);
    if (n + m == 0) return FS_OK;
    // before the first step the state lives in pos/vel (import); afterwards pos/vel hold the advanced state
    launch_slab_export(s->stream, P, s->slab_arrays());
    if (n) FS_HIP(hipMemcpyAsync(dst, s->aos.p, n * sizeof(fs_particle), hipMemcpyDeviceToHost, s->stream));
    if (n) FS_HIP(hipMemcpyAsync(owned, s->owned.p, n, hipMemcpyDeviceToHost, s->stream));
    if (m) FS_HIP(hipMemcpyAsync(dst + n, s->aos.p + S.main_slots, m * sizeof(fs_particle), hipMemcpyDeviceToHost, s->stream));
    if (m) FS_HIP(hipMemcpyAsync(owned + n, s->owned.p + S.main_slots, m, hipMemcpyDeviceToHost, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    return FS_OK;
}

fs_status fs_slab_column_histogram(fs_sim* s, uint32_t* hist, size_t grid_w_global) {
    if (!s || !s->slab || !hist || grid_w_global < s->grid_w) return fail(FS_ERR_INVALID, "bad argument");
    SlabState& S = *s->slab;
    FS_JOIN(s);
    FS_HIP(hipSetDevice(s->device));
    const StepParams P = params_of_state(*s);
    FS_HIP(hipMemsetAsync(S.hist.p, 0, S.hist.n * sizeof(uint32_t), s->stream));
    launch_slab_colhist(s->stream, P, s->slab_arrays(), S.hist.p, S.migrant_slots());
    std::vector<uint32_t> tmp(s->grid_w);
    FS_HIP(hipMemcpyAsync(tmp.data(), S.hist.p, tmp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    FS_HIP(hipStreamSynchronize(s->stream));
    for (uint32_t c = P.own_lo; c < P.own_hi; ++c) hist[c] = tmp[c];
    return FS_OK;
}

}  // extern "C"
