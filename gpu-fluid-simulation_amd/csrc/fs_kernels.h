// fs_kernels.h — host-side launchers of the HIP kernels (kernels_*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "fs_count.h"
#include "fs_device.h"

namespace fsd {

// Grids of the 256-thread kernels (FS_BLOCK, fs_neighbours.h) over n particles.
static inline uint32_t nblk(uint32_t n) { return (n + 256u - 1u) / 256u; }
static inline uint32_t xcd_grid(uint32_t nb, uint32_t c) {      // blocks to launch for xcd_block() (fs_device.h)
    const uint32_t chunks = (nb + (1u << c) - 1u) >> c;
    return (((chunks + 7u) >> 3) << 3) << c;
}

// The device arrays the sort-reorder, density, surface-tension and force passes of ONE particle array read and write (the main
// array of a handle, or the boundary strip of an overlapped slab step).  Fields carry the name of the role the passes see;
// a handle fills the set in one place and a call site overrides what differs for its launch.  Host side only: the launchers
// unpack it into the kernels' own parameter lists.
struct StepArrays {
    const float2* pos = nullptr;       // state before the step (cell order of the last step): what the reorder passes gather from
    const float2* vel = nullptr;
    float2* pos_s = nullptr;           // cell-sorted snapshot the density / force passes read (Jacobi semantics); pos_s == nullptr:
    float2* vel_s = nullptr;           //   the reorder pass keeps no sorted copy of the positions (StepParams::pos_by_src)
    float2* pred = nullptr;            // sorted predicted positions, + FS_PRED_SLACK entries
    float* rho = nullptr;              // densities; nullptr: the density pass leaves them in rho2.x only (strict / ulp modes)
    float2* rho2 = nullptr;            // {rho, +-RN(1/rho)}: the sign is the particle's safe-operand classification
    u64* pairs = nullptr;              // sorted (key << 32 | source slot)
    uint32_t* cs = nullptr;            // dense cell-start table, ncell + 1
    uint32_t* start_ref = nullptr;     // reference start_indices (persistent, never cleared)
    unsigned long long* safe = nullptr;   // kin_safe: one bit per sorted particle, a word per wave
    uint32_t* fdefer = nullptr;        // force pass: per-block deferred-wave bits, two words per 256-particle block
    uint32_t* fwork = nullptr;         // ... its worklist (per block)
    uint32_t* fcount = nullptr;        // ... and its work counters [2]: pre-registered waves
    float2* pos_out = nullptr;         // the force pass's output: the new state
    float2* vel_out = nullptr;
    const float2* tex = nullptr;       // obstacle push-out field
    uint32_t* key_s = nullptr;         // sorted keys, or nullptr: they stay in the high words of `pairs` only
    unsigned char* owned = nullptr;    // slab reorders: owned flag per sorted slot
    uint32_t* csort = nullptr;         // counting sort: its scratch (launch_counting_reorder*)
    const uint32_t* n_dev = nullptr;   // launch_counting_reorder_slab: device word holding the number of slots in use (<= cap;
                                       //   the grids still cover `cap`), or nullptr
    void* work = nullptr;              // network sort: the gap worklist of the reorder pass ...
    uint32_t* counter = nullptr;       // ... and its counter
};

void launch_reorder(hipStream_t st, const StepParams& P, const StepArrays& A, uint32_t work_cap, bool cs_ready = false);
// the chunked sweep of k_force reads up to 35 candidates past a row range when it scans global memory
#define FS_PRED_SLACK 64
void launch_density(hipStream_t st, const StepParams& P, const StepArrays& A,
                    uint32_t edge_grid = 0 /* != 0: edge-first slab step, column-major ids: only the blocks of the edge columns (+1), walked by this many workgroups */);
// Per-launch choices of the force pass (not state): name what a call site sets.
struct ForceLaunch {
    void* aos_out = nullptr;           // 32-B ParticleInstance records, or none
    hipStream_t side = nullptr;        // second stream: the pre-registered general work runs beside the lean kernel
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    uint32_t general_grid = 0;         // workgroups of the general kernel; 0: the full grid
    uint32_t* general_hint = nullptr;  // host-visible word: entries the general kernel found in its lists
    uint32_t edge_grid = 0;            // != 0: the lean kernel walks only the blocks of the edge columns with this many workgroups
    hipEvent_t done = nullptr;         // completes with the LAST launch of the pass (its own completion signal: no marker packet)
    uint32_t quad_entries = 0;         // != 0: the pre-registered list is expected to hold about this many blocks, few enough for
                                       // k_force_quad (four lanes per particle)
    const float2* st_in = nullptr;     // != nullptr (single-domain handles): the surface-tension force of each sorted slot,
                                       // launch_surface_tension's output, is added to the force sum (the ST instantiations)
};
void launch_force(hipStream_t st, const StepParams& P, const StepArrays& A, const ForceLaunch& L = ForceLaunch());
// Surface tension (build extension): st_out[i] = the colour-field CSF force of sorted slot i, from this step's
// densities (rho2; A.rho != nullptr: tolerance mode, densities in rho) over the density pass's neighbour walk.  Single-domain handles.
// cg = poly6_kernel_derivative (24/(pi h^8)); sigma = surface_tension_coefficient, tau = surface_tension_treshold.
void launch_surface_tension(hipStream_t st, const StepParams& P, const StepArrays& A, float sigma, float tau, float cg, float2* st_out);
// Diffusion and buoyancy of the tracking channels (build extension; kernels_diffuse.hip), after launch_density and
// launch_surface_tension, before launch_force.  The plan of one step, by value: channel[0 .. count) are the diffusing channels,
// ascending, g[k] = (2 kappa) delta of channel[k]; buoyancy_channel >= 0: fb_out[i] = (st_in[i] +) (rho_i beta (reference - A_b[i]))
// gravity, which the force launch takes as ForceLaunch::st_in.  attr_in: the channels as the carry delivered them (channel c at
// c * stride); attr_out: the spare set, of which only the rows of the diffusing channels are written.  cg, A.rho: as for
// launch_surface_tension.  count == 0 and no buoyancy channel: no launch.
struct DiffusePlan {
    int count = 0;
    int channel[4] = {0, 0, 0, 0};
    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int buoyancy_channel = -1;
    float beta = 0.0f, reference = 0.0f, gravity_x = 0.0f, gravity_y = 0.0f;
};
void launch_diffuse(hipStream_t st, const StepParams& P, const StepArrays& A, const DiffusePlan& D, float cg, const float* attr_in,
                    float* attr_out, uint32_t stride, const float2* st_in, float2* fb_out);
// The opt-in moving bodies of a single-domain handle (include/fluidsim.h "2D moving bodies") as k_bodies takes
// them, by value and apart from StepParams (kernels_bodies.hip).  Per body: the field of push vectors over the body's own box,
// and the motion of this enqueue.  rij: row-major R, world = R * local.  body[0 .. count) are the slots in use, ascending.
constexpr uint32_t BODIES2_MAX = 8u;   // FS_MAX_BODIES
struct Body2 {
    const float2* field;
    uint32_t w, h;
    float ex, ey;                      // the box's extent: the divisor of the lookup
    float hx, hy;                      // extent * 0.5f
    float cx, cy;
    float r00, r01, r10, r11;
    float ux, uy;
    float wz;
};
struct Bodies2 {
    uint32_t count;
    Body2 body[BODIES2_MAX];
};
// After launch_force, on the positions (A.pos_out) and velocities (A.vel_out) it stored: the operators B of every body in order.
// P: n, bs_x, bs_y, damping.  aos (may be null): the 32-B records the force pass wrote as well (ForceLaunch::aos_out); a particle
// a body hits gets its new position and velocity there too.  done (may be null): signalled by the kernel's completion, as
// ForceLaunch::done is.
void launch_bodies(hipStream_t st, const StepParams& P, const StepArrays& A, const Bodies2& B, void* aos, hipEvent_t done);
// The same pass while the handle's loads are on (include/fluidsim.h "2D body loads"): k_bodies_loads, which also
// adds each body's five 64-bit words of this step (sum Q(j.x), sum Q(j.y), sum Q(tz), hits, dropped; by kernel index) into a
// row of `shards` (BODY_LOAD_SHARDS rows of BODY_LOAD_ROW words, all zero on entry), then k_body_loads_fold, which adds the rows
// into `words` (FS_MAX_BODIES x 5, by slot: M.slot[kernel index]) and leaves `shards` zero again; the fold carries `done`.
constexpr uint32_t BODY_LOAD_SHIFT = 20u;      // FS_BODY_LOAD_SHIFT
constexpr uint32_t BODY_LOAD_WORDS = 5u;
constexpr uint32_t BODY_LOAD_ROW = BODIES2_MAX * BODY_LOAD_WORDS;
constexpr uint32_t BODY_LOAD_SHARDS = 64u;
struct BodyLoadMap {
    uint32_t count;                    // Bodies2::count
    uint32_t slot[BODIES2_MAX];
};
void launch_bodies_loads(hipStream_t st, const StepParams& P, const StepArrays& A, const Bodies2& B, void* aos, const BodyLoadMap& M,
                         unsigned long long* shards, unsigned long long* words, hipEvent_t done);
// Particle tracking (build extension): after the reorder pass of a step, id_out[i] = id_in[src] and, for c < channels,
// attr_out[c * stride + i] = attr_in[c * stride + src], src = the low word of pairs[i] (the slot before the step).  channels in [0, 4].
void launch_track_carry(hipStream_t st, uint32_t n, int channels, const u64* pairs, const uint32_t* id_in, uint32_t* id_out,
                        const float* attr_in, float* attr_out, uint32_t stride);
void launch_track_iota(hipStream_t st, uint32_t n, uint32_t* id);   // id[i] = i
// pairs != nullptr: the keys are the high words of the sorted pairs (the state of the last step; launch_reorder with
// key_s == nullptr does not store them a second time), else `key` (an uploaded state).
void launch_export_aos(hipStream_t st, uint32_t n, const float2* pos, const float2* pred, const float2* vel,
                       const float* rho, const uint32_t* key, void* out, const u64* pairs = nullptr,
                       const float2* rho2 = nullptr /* != nullptr: densities are rho2[i].x (launch_density with rho == nullptr) */);
// key[i] = pairs[i] >> 32 (pairs != nullptr), rho[i] = rho2[i].x (rho2 != nullptr): the copies the step no longer writes
void launch_keys_from_pairs(hipStream_t st, uint32_t n, const u64* pairs, uint32_t* key, const float2* rho2, float* rho);
void launch_import_aos(hipStream_t st, uint32_t n, const void* in, float2* pos, float2* pred, float2* vel, float* rho,
                       uint32_t* key);
// A particle count that changes at run time: fs_count.h.

void launch_render_density(hipStream_t st, const StepParams& P, float2 wmin, float2 wmax, uint32_t width,
                           uint32_t height, const float2* pred, const float2* vel, const uint32_t* cs,
                           const uint32_t* start_ref, const u64* pairs, float4* out);
// Field sampling (build extension; kernels_sample.hip): density, Shepard weight, velocity and channel sums of the
// state the last step left (SampleState) at the points of a SampleQuery.  All pointers are device pointers.
struct SampleQuery {
    uint32_t n = 0;                    // queries; with points == nullptr: width * height
    const float2* points = nullptr;    // nullptr: the pixel centres of the view below (fs_render_density's mapping), row-major
    float2 wmin = {0.0f, 0.0f}, wmax = {0.0f, 0.0f};
    uint32_t width = 0, height = 0;
    void* out = nullptr;               // n fs_sample records (24 B)
    float* attr_out = nullptr;         // channels * n floats, channel c at c * n; unused with channels == 0
};
struct SampleState {
    const float2* pred = nullptr;      // sorted predicted positions
    const float2* vel = nullptr;       // the step's new velocities
    const float2* rho2 = nullptr;      // {rho, +-RN(1/rho)} (strict / ulp step) ...
    const float* rho = nullptr;        // ... or, != nullptr, the densities themselves (tolerance step)
    const uint32_t* cs = nullptr;
    const uint32_t* start_ref = nullptr;
    const u64* pairs = nullptr;
    int channels = 0;                  // 0: no channel sums
    const float* attr = nullptr;       // channel c at attr + c * attr_stride
    uint32_t attr_stride = 0;
};
void launch_sample(hipStream_t st, const StepParams& P, const SampleQuery& Q, const SampleState& S);
// Fluid diagnostics (build extension, include/fluidsim.h "fluid diagnostics"; kernels_stats.hip, device helpers
// fs_stats.h): k_stats reads the arrays a download would export, in place, and stores one row of stats_words(2) 64-bit words per
// block into `slab` (at most STATS_MAX_BLOCKS rows; nothing in it needs to be zero); k_stats_fold reduces the rows and writes the
// 208-byte fs_stats record to `out`.  Device pointers; `out` is 8-byte aligned.
constexpr uint32_t STATS_SHIFT = 20u;          // FS_STATS_SHIFT
constexpr uint32_t STATS_THREADS = 256u;
constexpr uint32_t STATS_CHUNK = 512u;         // particles a block takes per trip of its stride loop: two per lane
constexpr uint32_t STATS_MAX_BLOCKS = 2048u;   // the grid cap (tests/test_stats_gpu.py states it too)
constexpr uint32_t stats_words(int dims) { return 4u * (uint32_t)dims + 23u; }     // 31 in 2D, 35 in 3D (fs_stats.h has the layout)
inline uint32_t stats_blocks(uint32_t n) {
    const uint32_t chunks = (n + STATS_CHUNK - 1u) / STATS_CHUNK;
    return chunks == 0u ? 1u : chunks < STATS_MAX_BLOCKS ? chunks : STATS_MAX_BLOCKS;
}
struct StatsInput {
    uint32_t n = 0;
    const float2* pos = nullptr;       // what launch_export_aos reads
    const float2* vel = nullptr;
    const float* rho = nullptr;        // the densities ...
    const float2* rho2 = nullptr;      // ... or, != nullptr, {rho, +-RN(1/rho)} (a strict / ulp step)
    int channels = 0;                  // 0 .. FS_TRACK_MAX_CHANNELS
    const float* attr = nullptr;       // channel c at attr + c * attr_stride
    uint32_t attr_stride = 0;
    uint32_t tick = 0;
};
void launch_stats(hipStream_t st, const StatsInput& I, unsigned long long* slab, void* out);
// The fold alone, for `rows` rows of stats_words(dims) words: the 3D launcher's second launch (kernels_stats3d.hip) is this one.
void launch_stats_fold(hipStream_t st, int dims, const unsigned long long* slab, uint32_t rows, uint32_t n, uint32_t tick,
                       int channels, void* out);
// Obstacle push-out field (kernels_field.hip); h <= 1024, w < 65536.
void launch_gradient_field(hipStream_t st, const unsigned char* image, uint32_t w, uint32_t h, float* dist,
                           uint32_t* nearest, float2* field);
// Exhaustive proof of fs_device.h div_const_fast over lo <= |x| <= hi (both signs).
#define FS_CONSTDIV_MIN 8.67361737988403547e-19f   /* 2^-60 */
void launch_verify_constdiv(hipStream_t st, float c, float y, float lo, float hi, uint32_t* mismatches);
void launch_verify_unary(hipStream_t st, int which /* 0 rcp_rn_fast, 1 sqrt_rn_fast */, float lo, float hi,
                         uint32_t* mismatches);
size_t gap_entry_size();
void launch_fill_gaps(hipStream_t st, uint32_t* cs, const void* work, const uint32_t* counter, uint32_t work_cap);

// ---- slab (multi-GPU) mode, kernels_slab.hip / kernels_strip.hip -------------------------------------------------
// The arrays of a slab handle its launchers work on: the main array's step arrays (the state is read through pos / vel and
// written through pos_out / vel_out, the same arrays; key_s: the sorted keys of the last step or import) and the slab's own,
// filled in one place on the handle (engine.h).  Host side only.
struct SlabArrays : StepArrays {
    uint32_t cap = 0, main_slots = 0;  // all slots; those before the 2R slots that mirror the incoming messages
    bool counting = true, overlap = false;   // the handle's sort: the counting sort, or the network; its step: the strips step (the
                                             // slots past main_slots hold last step's migrants)
    void* aos = nullptr;               // 32-B records: import / export staging
    u64* out = nullptr;                // the counting sort's (key, ticket) words (counting_sort_kt) or, in bitonic mode, the pairs
    uint32_t* hist = nullptr;          // the counting sort's histogram (counting_sort_hist)
    void* blockcnt = nullptr;          // one uint2 per 256-slot block, twice: message counts, then message offsets (k_slab_msg)
    uint32_t* stage = nullptr;         // slab_stage_words(cap) words
    void* msg_state = nullptr;         // one u64 per slab_msg_groups(cap) (look-back)
    uint32_t* counters = nullptr;      // [0] n_live, [2] lost, [3] overflow, [4] far_halo, [5] max-speed bits, [6] the look-back's ticket
};
// One set of halo messages: the outgoing pair a pack launch fills, or the incoming pair an unpack launch reads.
struct SlabMessages {
    uint32_t R = 0;                    // records per message (recv_capacity)
    int has_left = 0, has_right = 0;
    void *left = nullptr, *right = nullptr;   // nullptr: no neighbour on that side
    uint32_t epoch = 0;                // outgoing: a number unique to the launch among the handle's k_slab_msg launches
};
// Columns of one overlapped step (engine_slab.hip plan_overlap): [adv_lo, adv_hi) = the interior columns (global), advanced while
// the messages are in flight; win = the two strip windows as LOCAL column ranges [win[0], win[1]) and [win[2], win[3]).
struct OverlapPlan {
    uint32_t adv_lo = 0, adv_hi = 0;
    uint32_t win[4] = {0, 0, 0, 0};
    bool strip_active = false;
};
// Per-launch choices of launch_slab_pack.
struct SlabPack {
    bool lists = true;                 // false: the messages were pre-built (launch_slab_prepack): only check that every particle
                                       // the full classification flags was in the edge zone [own_lo, prev_adv_lo) u [prev_adv_hi, own_hi)
                                       // of the last step (key_s: its sorted keys)
    uint32_t prev_adv_lo = 0, prev_adv_hi = 0;
    bool skip_edge = false;            // with lists == false: the slots of the last step's edge-zone particles were classified by
                                       // launch_slab_prepack(classify) already — leave them alone
};
void launch_slab_pack(hipStream_t st, const StepParams& P, const SlabArrays& A, const SlabMessages& M, const SlabPack& O);
// Edge-first step: the NEXT step's messages from the particles the StepParams::adv_outside force launch has just advanced.
// `P_next`: window + tick constants of the next pack, adv_* as in that force launch.
void launch_slab_prepack(hipStream_t st, const StepParams& P_next, const SlabArrays& A, const SlabMessages& M,
                         uint32_t edge_grid = 0 /* != 0 (column-major ids): walk only the edge columns' blocks */,
                         bool classify = false /* also do the next launch_slab_pack's work for the slots of the particles it takes:
                                                  key, histogram ticket (counting sort) and out[] entry, the lost counter */);
// Overlapped slab step — the boundary strips (kernels_strip.hip).  `P` = the main array's StepParams, `A` its arrays;
// StripArrays::counters: [0] live strip particles (written by the strip's scan), [1] slots filled from the main array, [2] slots in use.
struct StripArrays {
    uint32_t cap = 0;
    float2 *pos = nullptr, *vel = nullptr;   // the strip's own particle array before its step ...
    u64* kt = nullptr;                 // ... its counting sort's words and histogram
    uint32_t* hist = nullptr;
    uint32_t* back = nullptr;          // main-array slot of each strip slot
    uint32_t* rowbase = nullptr;       // 2 * grid_h
    unsigned long long* safe = nullptr;
    uint32_t* counters = nullptr;
    const u64* pairs = nullptr;        // after its step: what the write-back scatters into the main array
    const float2 *pos_out = nullptr, *vel_out = nullptr, *pred = nullptr;
    const float* rho = nullptr;
};
void launch_strip_gather(hipStream_t st, const StepParams& P, const SlabArrays& A, const StripArrays& T, const OverlapPlan& plan, uint32_t R);
void launch_strip_unpack(hipStream_t st, const StepParams& P, const SlabArrays& A, const StripArrays& T, const SlabMessages& M);
void launch_strip_writeback(hipStream_t st, const StepParams& P_strip, const SlabArrays& A, const StripArrays& T);
size_t slab_stage_words(uint32_t cap);
size_t slab_msg_groups(uint32_t cap);
void launch_slab_unpack(hipStream_t st, const StepParams& P, const SlabArrays& A, const SlabMessages& M);
void launch_slab_reorder(hipStream_t st, const StepParams& P, const SlabArrays& A, uint32_t work_cap);
void launch_slab_export(hipStream_t st, const StepParams& P, const SlabArrays& A);
void launch_slab_import(hipStream_t st, const StepParams& P, const SlabArrays& A, uint32_t n);
// migr_count: the migrant slots of an overlapped step (outside the sorted prefix, from SlabArrays::main_slots), or 0
void launch_slab_colhist(hipStream_t st, const StepParams& P, const SlabArrays& A, uint32_t* hist_global, uint32_t migr_count);
// the bits of the largest owned |velocity| into counters[5]
void launch_slab_maxspeed(hipStream_t st, const SlabArrays& A, uint32_t migr_count);
size_t slab_message_bytes(uint32_t R);

// ---- the bitonic sort (kernels_sort.hip: the schedule; kernels_sort_tile.inc, kernels_sort_global.inc: its kernels) ----
// Late-stage plan of one sort call (kernels_sort_global.inc, k_late_cert).  Whatever the plan, the result is the network's.
struct SortPlan {
    int fuse_stage = -1;           // < 0: default stage, 0: per-stage launches only, k: the shifted merge from stage k
    int fallback = 0;              // what stands by for a failing certificate: 0 the per-stage launches (each returns at
                                   // once when not needed, ~5 us apiece), 1 one persistent launch (slow when it has work)
    uint32_t* feedback = nullptr;  // host-visible words the certificate reports to (stage, verdict, fit class, seq), or none
    uint32_t seq = 0;
    int inject_timeout = 0;        // tests (FS_SORT_INJECT_TIMEOUT=1): the stand-by kernel reports a barrier time-out it did not have
};
// What the 3D predict + cell key needs (fs_3d.h predict3 / cell_key3).
struct KeyGen3 { float dt, h, bx, by, bz; uint32_t gw, gh; };
// The state a sort call builds its pairs from (no SortKeys: `pairs` holds them): the first kernel computes predict + cell
// key itself (fused into its tile load, compute.wgsl:8-42) and clears `gap_counter` for the reorder pass that follows in
// the stream.  Held in the form the kernels' parameter list has — one StepParams and float2 arrays — so the 3D
// constructor is the one place where the 3D parameters and arrays are dressed up as the 2D ones; k_bitonic_local and
// k_bitonic_local32 undo it with the matching casts when KEYGEN == 2.
struct SortKeys {
    int keygen;                    // the kernels' KEYGEN argument: 1 = 2D, 2 = 3D
    StepParams P;
    const float2 *pos, *vel;
    uint32_t* gap_counter;
    SortKeys(const StepParams& P2, const float2* pos2, const float2* vel2, uint32_t* gap)
        : keygen(1), P(P2), pos(pos2), vel(vel2), gap_counter(gap) {}
    SortKeys(const KeyGen3& K, const float4* pos4, const float4* vel4, uint32_t* gap)
        : keygen(2), pos(reinterpret_cast<const float2*>(pos4)), vel(reinterpret_cast<const float2*>(vel4)), gap_counter(gap) {
        static_assert(sizeof(KeyGen3) <= sizeof(StepParams), "KeyGen3 rides in the StepParams argument");
        memset(&P, 0, sizeof P);
        memcpy(&P, &K, sizeof K);
    }
};
// Bitonic network of sort.wgsl:27-51 / simulation.rs:323-347 on (key<<32 | index) pairs.
// Returns the number of kernel launches issued.
// `dirty`: one u32 per 4096-element tile and, behind them, the plan words (sort_tile_count(n) entries; fs_sort.h
// SortPlanWord), scratch owned by the caller, zero at create.
int launch_bitonic_sort(hipStream_t st, u64* pairs, uint32_t n, uint32_t* dirty, const SortKeys* keys = nullptr,
                        const SortPlan* plan = nullptr);
uint32_t sort_tile_count(uint32_t n);      // entries of `dirty` for a sort of n elements
uint32_t sort_plan_word(uint32_t n);       // index of the first plan word in it

// FS_SORT_COUNTING (kernels_csort.hip).  The scratch must be all-zero when the handle is created (histogram, tickets);
// every step leaves it that way.  `epoch`: a number unique to the launch among the handle's launches.
//   single domain: launch_counting_sort (hist -> scan -> scatter: fills `cs`) + launch_counting_reorder (rank fix-up fused
//   with the whole reorder pass: fills `pairs`, pos_s / vel_s / pred_s, start_ref, safe bits);
//   slabs: k_slab_pack / k_slab_unpack fill the histogram, then launch_counting_sort_pairs (scan -> scatter; live count)
//   + launch_counting_reorder_slab.
size_t counting_sort_scratch_words(uint32_t n, uint32_t ncell_max);
u64* counting_sort_kt(uint32_t* scratch, uint32_t n, uint32_t ncell_alloc);
uint32_t* counting_sort_hist(uint32_t* scratch);
// `cap` (>= P.n): the slots the scratch was sized for.  Everything behind the histogram is placed by it, not by P.n, so that
// a count that changes at run time moves nothing: with cap == P.n the addresses are those of a fixed count.
void launch_counting_sort(hipStream_t st, const StepParams& P, uint32_t cap, const float2* pos, const float2* vel, uint32_t* cs,
                          uint32_t* scratch, uint32_t* gap_counter, unsigned long long* safe, uint32_t epoch);
void launch_counting_reorder(hipStream_t st, const StepParams& P, uint32_t cap, const StepArrays& A);
// n_dev (may be null): as StepArrays::n_dev
void launch_counting_sort_pairs(hipStream_t st, uint32_t cap, uint32_t ncell, uint32_t ncell_alloc, uint32_t* cs, uint32_t* scratch,
                                uint32_t* n_live_out, uint32_t epoch, const uint32_t* n_dev = nullptr,
                                unsigned long long* safe_preset = nullptr /* the slots' "safe operand" words, set to all-ones for k_cs_fixreorder */);
void launch_counting_reorder_slab(hipStream_t st, const StepParams& P, const StepArrays& A, uint32_t cap, uint32_t ncell_alloc,
                                  hipEvent_t done = nullptr /* signalled by the kernel's completion */);

}  // namespace fsd
