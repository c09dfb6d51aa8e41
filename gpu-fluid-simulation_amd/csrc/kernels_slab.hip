// kernels_slab.hip — multi-GPU slab mode (NOT in the reference, which is
// single-device).  A rank owns the global cell columns [own_lo, own_hi) and keeps a
// fixed-capacity local array whose slots are either live particles or DEAD (key
// 0xFFFFFFFF).  Everything a step needs to know about counts lives on the device, so a
// step is enqueued without any host synchronisation:
//
//   slots [0, main)            particles carried over from the last step (owned + old ghosts)
//   slots [main, main+R)       records received from the left neighbour this step
//   slots [main+R, main+2R)    records received from the right neighbour this step
//
// An outgoing message pair is built by three kernels:
//   k_slab_pack      predict + global column of every carried-over owned particle; old ghosts and leavers become DEAD.
//                    Counting sort: the key goes straight into the sort's histogram and the atomic's return value, the
//                    particle's arrival ticket in its cell, is stored beside it (kt[i] = key << 32 | ticket, fs_scan.h
//                    cell_ticket), so the sort needs no pass of its own over the slots; bitonic: pairs[i] = key << 32 | i.
//                    The slots each neighbour needs (migrants + the 2-column halo) are listed per 256-slot block, in slot
//                    order (stage_l / stage_r, 256 entries per block), with the two counts in blockcnt[block].
//                    (k_slab_prepack: the same for the next step, from the edge columns alone — the edge-first step.)
//   k_slab_msg       one wave per MSG_GROUP blocks: exclusive message offsets of its blocks by a wave scan + a decoupled
//                    look-back over the (few) groups (fs_scan.h); the last group writes the two headers.
//   k_slab_gather    one workgroup per block: its listed records -> the two fixed-size messages [16-B header | R x {pos, vel}],
//                    in SLOT ORDER (deterministic).
// Why three.  A look-back over the 256-slot blocks themselves, one launch, has a prefix frontier that advances ~128 blocks per
// global-memory round trip: 0.17 ms for the 11 136 blocks of an 8-way rank — the chain must be short, hence the groups.  And
// a group that gathers the records of its own 64 blocks is fine only while the flagged slots are spread over the array: with
// column-major cell ids a rank's edge columns are ~80 CONSECUTIVE blocks per side, two workgroups then gather 20 000 records
// each, 50 - 67 us instead of the 8 us of one workgroup per block.
//
//   k_slab_unpack    received records -> slots, key from the recomputed predicted position (+ histogram ticket)
//   counting sort (default): k_scan_lookback -> k_cs_scatter -> k_cs_fixreorder<true> (kernels_csort.hip; the last one is
//                    the reorder pass as well: live count, owned flags, start_indices)
//   bitonic mode:    the network over all slots (DEAD keys end up last) + k_slab_reorder
//   k_density / k_force run unchanged on the local window (ghosts are not advanced)
// The strips step's own kernels are in kernels_strip.hip; the device helpers all of these share in fs_slab.h.
#include "fs_device.h"
#include "fs_kernels.h"
#include "fs_scan.h"
#include "fs_slab.h"

namespace fsd {

// The per-block lists and counts of the pack (flag bit 0: left message, bit 1: right): the input of k_slab_msg.  Whole workgroup.
__device__ __forceinline__ void block_message_lists(unsigned char f, uint32_t i, uint32_t blk, uint2* __restrict__ blockcnt,
                                                    uint32_t* __restrict__ stage_l, uint32_t* __restrict__ stage_r) {
    __shared__ uint32_t s_cnt[2 * (SL_BLOCK / 64)];
    const unsigned long long mL = __ballot(f & 1), mR = __ballot(f & 2);
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    if (lane == 0) { s_cnt[2 * w] = __popcll(mL); s_cnt[2 * w + 1] = __popcll(mR); }
    __syncthreads();
    uint32_t wl = 0, wr = 0, tl = 0, tr = 0;
#pragma unroll
    for (uint32_t k = 0; k < SL_BLOCK / 64; ++k) {
        const uint32_t a = s_cnt[2 * k], b = s_cnt[2 * k + 1];
        if (k < w) { wl += a; wr += b; }
        tl += a; tr += b;
    }
    if (threadIdx.x == 0) blockcnt[blk] = make_uint2(tl, tr);
    if (f) {
        const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
        if (f & 1) stage_l[blk * SL_BLOCK + wl + __popcll(mL & below)] = i;
        if (f & 2) stage_r[blk * SL_BLOCK + wr + __popcll(mR & below)] = i;
    }
}

// overlap != 0 (the strips step, engine_slab.hip): ghosts never enter the main array, so the slots past `main_slots` are not the
// unpack area of this step but hold the MIGRANTS the boundary strips received and advanced in the last one (owned flag
// set by k_strip_writeback); they are carried over like the sorted prefix.
template <bool COUNTING>
__global__ __launch_bounds__(SL_BLOCK) void k_slab_pack(StepParams P, uint32_t cap, uint32_t main_slots, int overlap, int lists,
                                                        int has_left, int has_right, const float2* __restrict__ pos,
                                                        const float2* __restrict__ vel,
                                                        const unsigned char* __restrict__ owned, u64* __restrict__ out /* kt or pairs */,
                                                        uint32_t* __restrict__ hist, uint2* __restrict__ blockcnt,
                                                        uint32_t* __restrict__ stage_l, uint32_t* __restrict__ stage_r,
                                                        uint32_t* __restrict__ counters, uint32_t* __restrict__ gap_counter,
                                                        const uint32_t* __restrict__ key_prev, uint32_t prev_adv_lo,
                                                        uint32_t prev_adv_hi, int skip_edge) {
    const uint32_t i = blockIdx.x * SL_BLOCK + threadIdx.x;
    if (i == 0) *gap_counter = 0;          // cell-table worklist of this step (bitonic mode: k_slab_reorder)
    const uint32_t n_prev = *P.n_live;
    unsigned char f = 0;
    uint32_t key = FS_DEAD_KEY;
    if (overlap && i == 0 && n_prev > main_slots) atomicAdd(&counters[3], 1u);   // the sorted prefix ran into the migrant slots
    // lists == 0 (the messages were pre-built): where was this particle in the last step?  In the edge zone — then the edge
    // columns' chain of that step advanced it, put it into the messages and, with skip_edge, classified its slot for this step's
    // sort as well (k_slab_prepack: this launch then neither reads nor writes anything of it, and need not wait for that chain)
    bool was_edge = false, skipped = false;
    if (!lists && i < main_slots && i < n_prev && owned[i]) {
        const int32_t cg = global_col(P, key_prev[i]);
        was_edge = owns_col(P, cg) && !(cg >= (int32_t)prev_adv_lo && cg < (int32_t)prev_adv_hi);
        skipped = skip_edge && was_edge;
    }
    if (i < main_slots || (overlap && i < cap)) {
        if ((i < main_slots ? i < n_prev : true) && owned[i] && !skipped) {
            const float2 pr = predict_pos(P, pos[i], vel[i]);
            uint32_t cxg;
            key = slab_key(P, pr, &cxg);
            f = halo_flags(P, cxg, has_left, has_right);
            count_leavers(P, cxg, has_left, has_right, counters);
        }
        if (!COUNTING && !skipped) out[i] = ((u64)key << 32) | (u64)i;
    } else if (i < n_prev && i < cap && owned[i]) {
        // Slot capacity exceeded: the last step left more live records than main slots, and this owned particle sits where the
        // incoming messages will be unpacked.  It cannot be carried over: counted in overflow (the driver raises on it).
        atomicAdd(&counters[3], 1u);
    }
    if (COUNTING) {
        const bool active = key != FS_DEAD_KEY;
        const uint32_t ticket = cell_ticket(hist, key, P.ncell, active);
        if ((i < main_slots || (overlap && i < cap)) && !skipped) out[i] = ((u64)key << 32) | (u64)(active ? ticket : 0u);
    }
    if (lists) {
        block_message_lists(f, i, blockIdx.x, blockcnt, stage_l, stage_r);
    } else if (f && !was_edge) {
        // The messages of this step were built at the end of the last one, from the particles its edge-column force launch had
        // advanced by then (k_slab_prepack).  This full classification flags the same particles — unless one reached the 2-column
        // band from farther inside than the edge zone (its key of the last step says where it was): then the message that went
        // out lacks it.  Counted in far_halo (the edge zone was too narrow for its speed: fs_slab_set_boundary_cols).
        atomicAdd(&counters[4], 1u);
    }
}

// Edge-first step (engine_slab.hip): the messages of step t+1 are built at the END of step t, as soon as the force pass
// has advanced the owned columns within `boundary_cols` of a neighboured edge (StepParams::adv_outside launch) — the exchange
// then runs beside the force pass of the interior columns and the next step's k_slab_pack.  Same classification, same lists,
// same slot order as k_slab_pack would produce at t+1 (a particle's sorted index now IS its slot then), restricted to the
// particles that launch advanced; `P` carries the window and the tick constants the next pack will use.  The next k_slab_pack
// (lists = 0) checks the messages' completeness (far_halo).
__global__ __launch_bounds__(SL_BLOCK) void k_slab_prepack(StepParams P, int has_left, int has_right, int edge_walk,
                                                           const float2* __restrict__ pos, const float2* __restrict__ vel,
                                                           const unsigned char* __restrict__ owned,
                                                           const uint32_t* __restrict__ key_s, const uint32_t* __restrict__ cs,
                                                           uint2* __restrict__ blockcnt,
                                                           uint32_t* __restrict__ stage_l, uint32_t* __restrict__ stage_r,
                                                           int classify, int counting, uint32_t main_slots, u64* __restrict__ out,
                                                           uint32_t* __restrict__ hist, uint32_t* __restrict__ counters) {
    const uint32_t n = *P.n_live;
    // edge_walk (column-major ids): a small grid walks the blocks of the edge columns only (fs_device.h EdgeBlocks; k_slab_msg and
    // k_slab_gather take every other block's counts as zero); otherwise one workgroup per 256-slot block of the whole array
    const EdgeBlocks E = edge_blocks_or_all(P, edge_walk, cs, gridDim.x);
    const uint32_t count = edge_walk ? edge_block_count(E) : gridDim.x;
    for (uint32_t t = blockIdx.x; t < count; t += gridDim.x) {
        const uint32_t blk = edge_walk ? edge_block_at(E, t) : t;
        const uint32_t i = blk * SL_BLOCK + threadIdx.x;
        unsigned char f = 0;
        uint32_t key = FS_DEAD_KEY;
        bool mine = false;                                  // classify: this launch does the next pack's work for the slot
        if (i < n && owned[i] && slab_advances(P, global_col(P, key_s[i]))) {     // advanced already: pos / vel hold its new state
            uint32_t cxg;
            key = slab_key(P, predict_pos(P, pos[i], vel[i]), &cxg);
            f = halo_flags(P, cxg, has_left, has_right);
            mine = classify && i < main_slots;
            if (mine) count_leavers(P, cxg, has_left, has_right, counters);   // k_slab_pack will skip this slot
        }
        if (classify) {
            if (counting) {
                const bool active = mine && key != FS_DEAD_KEY;
                const uint32_t ticket = cell_ticket(hist, key, P.ncell, active);
                if (mine) out[i] = ((u64)key << 32) | (u64)(active ? ticket : 0u);
            } else if (mine) {
                out[i] = ((u64)key << 32) | (u64)i;
            }
        }
        block_message_lists(f, i, blk, blockcnt, stage_l, stage_r);
        __syncthreads();
    }
}

// Two message counters (records for the left / the right neighbour) travel through the look-back as one 40-bit payload
// of two saturating 20-bit fields: a count only matters up to R + 1 (overflow), and R < 2^20 - 2 (fs_slab_create).
#define PK_FIELD 0xFFFFFull
__device__ __forceinline__ u64 pk_add(u64 a, u64 b) {
    u64 l = (a >> 20) + (b >> 20), r = (a & PK_FIELD) + (b & PK_FIELD);
    if (l > PK_FIELD) l = PK_FIELD;
    if (r > PK_FIELD) r = PK_FIELD;
    return (l << 20) | r;
}

#define MSG_GROUP 64u        // pack blocks per k_slab_msg workgroup (one wave scans their counts)
// Per-block counts -> per-block message offsets (blockoff) + the two headers; k_slab_gather moves the records.  (It once
// gathered them itself, each workgroup for its 64 blocks: see the file header for what that cost.)
__global__ __launch_bounds__(64) void k_slab_msg(uint32_t nblocks_pack, uint32_t R, const uint2* __restrict__ blockcnt,
                                                 uint2* __restrict__ blockoff, u64* __restrict__ state,
                                                 uint32_t* __restrict__ ticket, uint32_t epoch, SlabHeader* hdr_left,
                                                 SlabHeader* hdr_right, uint32_t* __restrict__ counters, StepParams P,
                                                 const uint32_t* __restrict__ cs_edge) {
    __shared__ uint32_t s_bid;
    // cs_edge != null: only the edge columns' blocks were classified (k_slab_prepack with edge_walk); every other count is zero
    const EdgeBlocks E = edge_blocks_or_all(P, cs_edge, cs_edge, nblocks_pack);
    if (threadIdx.x == 0) s_bid = atomicAdd(ticket, 1u);
    __syncthreads();
    const uint32_t bid = s_bid, ngroups = gridDim.x;
    if (bid == ngroups - 1u && threadIdx.x == 0) *ticket = 0u;          // every ticket of this launch has been handed out
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = bid * MSG_GROUP + lane;
    const u64 tag = (u64)(epoch & 0x3FFFFFu);
    const uint2 c = (b < nblocks_pack && (!cs_edge || edge_block_has(E, b))) ? blockcnt[b] : make_uint2(0u, 0u);
    const uint32_t il = wave_inclusive_scan(c.x), ir = wave_inclusive_scan(c.y);
    const uint32_t tl = __shfl(il, 63), tr = __shfl(ir, 63);            // <= 64 * 256 each
    const u64 mine = ((u64)tl << 20) | (u64)tr;
    u64 ex = 0ull;
    if (bid == 0) {
        if (lane == 0) lb_store(state, (LB_FLAG_PREFIX << 62) | (tag << 40) | mine);
    } else {
        if (lane == 0) lb_store(state + bid, (LB_FLAG_AGG << 62) | (tag << 40) | mine);
        ex = lookback_exclusive<40>(state, bid, tag, pk_add);
        if (lane == 0) lb_store(state + bid, (LB_FLAG_PREFIX << 62) | (tag << 40) | pk_add(ex, mine));
    }
    const uint32_t offl = (uint32_t)(ex >> 20), offr = (uint32_t)(ex & PK_FIELD);
    if (b < nblocks_pack) blockoff[b] = make_uint2(offl + il - c.x, offr + ir - c.y);      // exclusive offsets of block b's records
    if (bid == ngroups - 1u && lane == 0) {                             // totals: the last group's inclusive prefix
        const uint32_t totl = offl + tl, totr = offr + tr;              // saturated at 2^20 - 1 > R
        if (hdr_left) { hdr_left->count = totl < R ? totl : R; hdr_left->overflow = totl > R; }
        if (hdr_right) { hdr_right->count = totr < R ? totr : R; hdr_right->overflow = totr > R; }
        if ((hdr_left && totl > R) || (hdr_right && totr > R)) atomicAdd(&counters[3], 1u);
    }
}

// The listed records of one pack block -> the two messages, in SLOT order (deterministic).
__global__ __launch_bounds__(SL_BLOCK) void k_slab_gather(uint32_t R, const uint2* __restrict__ blockcnt,
                                                          const uint2* __restrict__ blockoff,
                                                          const uint32_t* __restrict__ stage_l, const uint32_t* __restrict__ stage_r,
                                                          const float2* __restrict__ pos, const float2* __restrict__ vel,
                                                          float4* __restrict__ rec_left, float4* __restrict__ rec_right,
                                                          StepParams P, const uint32_t* __restrict__ cs_edge) {
    const EdgeBlocks E = edge_blocks_or_all(P, cs_edge, cs_edge, gridDim.x);
    const uint32_t count = cs_edge ? edge_block_count(E) : gridDim.x;
    for (uint32_t w = blockIdx.x; w < count; w += gridDim.x) {
        const uint32_t blk = cs_edge ? edge_block_at(E, w) : w;
        const uint2 c = blockcnt[blk];
        if ((c.x | c.y) == 0u) continue;
        const uint2 o = blockoff[blk];
        const uint32_t t = threadIdx.x;
        if (rec_left && t < c.x && o.x + t < R) {
            const uint32_t slot = stage_l[blk * SL_BLOCK + t];
            const float2 p = pos[slot], v = vel[slot];
            rec_left[o.x + t] = make_float4(p.x, p.y, v.x, v.y);
        }
        if (rec_right && t < c.y && o.y + t < R) {
            const uint32_t slot = stage_r[blk * SL_BLOCK + t];
            const float2 p = pos[slot], v = vel[slot];
            rec_right[o.y + t] = make_float4(p.x, p.y, v.x, v.y);
        }
    }
}

template <bool COUNTING>
__global__ __launch_bounds__(SL_BLOCK) void k_slab_unpack(StepParams P, uint32_t main_slots, uint32_t R,
                                                          const SlabHeader* __restrict__ hdr_left,
                                                          const float4* __restrict__ rec_left,
                                                          const SlabHeader* __restrict__ hdr_right,
                                                          const float4* __restrict__ rec_right,
                                                          float2* __restrict__ pos, float2* __restrict__ vel,
                                                          u64* __restrict__ out /* kt or pairs */, uint32_t* __restrict__ hist,
                                                          uint32_t* __restrict__ counters) {
    const uint32_t j = blockIdx.x * SL_BLOCK + threadIdx.x;
    const ReceivedRecord r(j, R, hdr_left, rec_left, hdr_right, rec_right, counters);
    const uint32_t slot = main_slots + j;
    uint32_t key = FS_DEAD_KEY, cxg;
    if (r.has()) key = r.read(P, &pos[slot], &vel[slot], counters, &cxg);
    if (COUNTING) {                                                     // received records join the histogram (after k_slab_pack's)
        const bool active = key != FS_DEAD_KEY;
        const uint32_t ticket = cell_ticket(hist, key, P.ncell, active);
        if (r.in_range) out[slot] = ((u64)key << 32) | (u64)(active ? ticket : 0u);
    } else if (r.in_range) {
        out[slot] = ((u64)key << 32) | (u64)slot;
    }
}

// k_reorder for slab mode: DEAD slots are skipped, the live count and the owned flags are
// produced here.  `cap` = number of slots sorted.
__global__ __launch_bounds__(SL_BLOCK) void k_slab_reorder(StepParams P, uint32_t cap, const u64* __restrict__ pairs,
                                                           const float2* __restrict__ pos_in,
                                                           const float2* __restrict__ vel_in,
                                                           float2* __restrict__ pos_s, float2* __restrict__ vel_s,
                                                           float2* __restrict__ pred_s, uint32_t* __restrict__ key_s,
                                                           unsigned char* __restrict__ owned,
                                                           uint32_t* __restrict__ cs, uint32_t* __restrict__ start_ref,
                                                           GapEntry* __restrict__ work, uint32_t* __restrict__ counter,
                                                           uint32_t work_cap, uint32_t* __restrict__ n_live_out,
                                                           unsigned long long* __restrict__ safe, uint32_t* __restrict__ force_defer,
                                                           uint32_t* __restrict__ force_work_count) {
    const uint32_t i = blockIdx.x * SL_BLOCK + threadIdx.x;
    if (threadIdx.x == 0) {                      // the force pass's worklists of this step (same block size)
        force_defer[2u * blockIdx.x] = 0u;
        force_defer[2u * blockIdx.x + 1u] = 0u;
        if (blockIdx.x == 0) { force_work_count[0] = 0u; force_work_count[1] = 0u; }
    }
    if (i >= cap) return;
    const u64 pr = pairs[i];
    const uint32_t key = (uint32_t)(pr >> 32);
    const uint32_t prev = i ? (uint32_t)(pairs[i - 1] >> 32) : 0u;
    if (key == FS_DEAD_KEY) {
        {   // the live count and the table come from here
            if (i == 0) { *n_live_out = 0; fill_cells(cs, 0u, P.ncell + 1u, 0u, work, counter, work_cap); }
            else if (prev != FS_DEAD_KEY) *n_live_out = i;
        }
        owned[i] = 0;
        return;
    }
    const uint32_t src = (uint32_t)pr;
    const float2 p = pos_in[src];
    const float2 v = vel_in[src];
    pos_s[i] = p;
    vel_s[i] = v;
    const float2 pd = predict_pos(P, p, v);
    pred_s[i] = pd;
    key_s[i] = key;
    {   // fs_device.h "safe operand" classification (finished by k_density): one 64-bit word per wave
        const unsigned long long sb = __builtin_amdgcn_ballot_w64(kin_safe(pd, v));   // lanes that returned above: 0
        if ((threadIdx.x & 63u) == 0u) safe[i >> 6] = sb;
    }
    owned[i] = owns_col(P, global_col(P, key)) ? 1 : 0;

    const uint32_t kc = key < P.ncell ? key : P.ncell;
    if (i == 0) {
        if (key < P.ncell) start_ref[key] = 0;
        fill_cells(cs, 0u, kc + 1u, 0u, work, counter, work_cap);
    } else if (key != prev) {
        if (key < P.ncell) start_ref[key] = i;
        const uint32_t pc = prev < P.ncell ? prev : P.ncell;
        fill_cells(cs, pc + 1u, kc + 1u, i, work, counter, work_cap);
    }
    {
        const bool last = (i + 1 == cap) || ((uint32_t)(pairs[i + 1] >> 32) == FS_DEAD_KEY);
        if (last) {
            fill_cells(cs, kc + 1u, P.ncell + 1u, i + 1u, work, counter, work_cap);
            if (i + 1 == cap) *n_live_out = cap;
        }
    }
}

struct AosParticle { float2 position, predicted, velocity; float density; uint32_t grid; };

// AoS export with GLOBAL cell keys (so results of different ranks / a single-GPU run compare).
__global__ __launch_bounds__(SL_BLOCK) void k_slab_export(StepParams P, uint32_t cap, const float2* __restrict__ pos,
                                                          const float2* __restrict__ pred,
                                                          const float2* __restrict__ vel,
                                                          const float* __restrict__ rho,
                                                          const uint32_t* __restrict__ key,
                                                          AosParticle* __restrict__ out) {
    const uint32_t i = blockIdx.x * SL_BLOCK + threadIdx.x;
    if (i >= cap) return;
    AosParticle a;
    a.position = pos[i]; a.predicted = pred[i]; a.velocity = vel[i]; a.density = rho[i];
    uint32_t cy;
    const int32_t cg = global_col(P, key[i], &cy);
    a.grid = cy * P.grid_w_global + (uint32_t)cg;                               // the reference's id (funcs.wgsl:216-218)
    out[i] = a;
}

// Initial owned particles: SoA import + owned flags + local keys.
__global__ __launch_bounds__(SL_BLOCK) void k_slab_import(StepParams P, uint32_t n, uint32_t cap,
                                                          const AosParticle* __restrict__ in,
                                                          float2* __restrict__ pos, float2* __restrict__ pred,
                                                          float2* __restrict__ vel, float* __restrict__ rho,
                                                          uint32_t* __restrict__ key, unsigned char* __restrict__ owned) {
    const uint32_t i = blockIdx.x * SL_BLOCK + threadIdx.x;
    if (i >= cap) return;
    if (i < n) {
        const AosParticle a = in[i];
        pos[i] = a.position; pred[i] = a.predicted; vel[i] = a.velocity; rho[i] = a.density;
        uint32_t cxg;
        key[i] = slab_key(P, a.predicted, &cxg);
        owned[i] = 1;
    } else {
        owned[i] = 0;
        key[i] = FS_DEAD_KEY;
    }
}

// Particles per GLOBAL column among the owned columns (for re-balancing): one thread per local column.
__global__ __launch_bounds__(SL_BLOCK) void k_slab_colhist(StepParams P, const uint32_t* __restrict__ cs,
                                                           uint32_t* __restrict__ hist_global) {
    const uint32_t c = blockIdx.x * SL_BLOCK + threadIdx.x;
    if (c >= P.grid_w) return;
    const int32_t cg = (int32_t)c + P.col_origin;
    if (!owns_col(P, cg)) return;
    uint32_t sum = 0;
    if (P.transposed) sum = cs[(c + 1u) * P.grid_h] - cs[c * P.grid_h];       // a column is one contiguous range of cell ids
    else for (uint32_t y = 0; y < P.grid_h; ++y) sum += cs[y * P.grid_w + c + 1] - cs[y * P.grid_w + c];
    atomicAdd(&hist_global[cg], sum);       // (the buffer was zeroed; k_slab_colhist_migrants adds to the same words)
}

// Overlapped step: the migrants a rank received and advanced in the last step sit in the slots past the main ones, outside
// the sorted prefix and its cell table; `key` holds their local cell key of that step.
__global__ __launch_bounds__(SL_BLOCK) void k_slab_colhist_migrants(StepParams P, uint32_t first, uint32_t count,
                                                                    const unsigned char* __restrict__ owned,
                                                                    const uint32_t* __restrict__ key,
                                                                    uint32_t* __restrict__ hist_global) {
    const uint32_t j = blockIdx.x * SL_BLOCK + threadIdx.x;
    if (j >= count || !owned[first + j]) return;
    const uint32_t k = key[first + j];
    if (k == FS_DEAD_KEY) return;
    const int32_t cg = global_col(P, k);
    if (cg >= 0 && cg < (int32_t)P.grid_w_global) atomicAdd(&hist_global[cg], 1u);
}

// Largest |velocity| among the owned live particles, as f32 bits (non-negative floats order like their bits):
// sizes the outer-edge margin between two re-balancing steps (multi.py).
__global__ __launch_bounds__(SL_BLOCK) void k_slab_maxspeed(const uint32_t* __restrict__ n_live,
                                                            const float2* __restrict__ vel,
                                                            const unsigned char* __restrict__ owned,
                                                            uint32_t* __restrict__ out_bits, uint32_t migr_first,
                                                            uint32_t migr_count) {
    const uint32_t n = *n_live;
    float m = 0.0f;
    // the sorted prefix [0, n), then (overlapped step) the migrant slots [migr_first, migr_first + migr_count)
    for (uint32_t t = blockIdx.x * SL_BLOCK + threadIdx.x; t < n + migr_count; t += gridDim.x * SL_BLOCK) {
        const uint32_t i = t < n ? t : migr_first + (t - n);
        if (t >= n && i < n) continue;                       // (a prefix that ran into the migrant slots: counted once)
        if (!owned[i]) continue;
        const float2 v = vel[i];
        const float sp = sqrt_rn(v.x * v.x + v.y * v.y);
        if (sp > m) m = sp;                                  // NaN never wins
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float t = __shfl_xor(m, o); m = t > m ? t : m; }
    if ((threadIdx.x & 63u) == 0 && m > 0.0f) atomicMax(out_bits, __float_as_uint(m));
}

// ------------------------------------------------------------------ launchers
void launch_slab_maxspeed(hipStream_t st, const SlabArrays& A, uint32_t migr_count) {
    hipLaunchKernelGGL(k_slab_maxspeed, dim3(1024), dim3(SL_BLOCK), 0, st, A.counters, A.vel, A.owned, A.counters + 5, A.main_slots, migr_count);
}

// The two halves of `stage` and the message headers, for `blocks` pack blocks.
struct MsgLayout {
    uint32_t blocks, groups;
    uint32_t *stage_l, *stage_r;
    SlabHeader *hl, *hr;
    MsgLayout(const SlabArrays& A, const SlabMessages& M, uint32_t cap)
        : blocks(sl_blocks(cap)), groups((blocks + MSG_GROUP - 1u) / MSG_GROUP), stage_l(A.stage), stage_r(A.stage + (size_t)blocks * SL_BLOCK),
          hl((SlabHeader*)M.left), hr((SlabHeader*)M.right) {}
};

// offsets + headers, then the parallel gather.  blockcnt holds 2 * (blocks + 1) entries: counts, then offsets.
static void launch_slab_msg(hipStream_t st, const StepParams& P, const SlabArrays& A, const SlabMessages& M, const MsgLayout& L,
                            const uint32_t* cs_edge = nullptr, uint32_t edge_grid = 0) {
    uint2* cnt = (uint2*)A.blockcnt;
    uint2* off = cnt + (L.blocks + 1u);
    hipLaunchKernelGGL(k_slab_msg, dim3(L.groups), dim3(64), 0, st, L.blocks, M.R, (const uint2*)cnt, off, (u64*)A.msg_state, A.counters + 6,
                       M.epoch, L.hl, L.hr, A.counters, P, cs_edge);
    hipLaunchKernelGGL(k_slab_gather, dim3(cs_edge ? edge_grid : L.blocks), dim3(SL_BLOCK), 0, st, M.R, (const uint2*)cnt, (const uint2*)off,
                       L.stage_l, L.stage_r, A.pos, A.vel, records(L.hl), records(L.hr), P, cs_edge);
}

void launch_slab_pack(hipStream_t st, const StepParams& P, const SlabArrays& A, const SlabMessages& M, const SlabPack& O) {
    // covers ALL slots (P.n = capacity): slots past `main_slots` only check for stranded owned particles
    const uint32_t cap = P.n > A.main_slots ? P.n : A.main_slots;
    const MsgLayout L(A, M, cap);
    hipLaunchKernelGGL(A.counting ? k_slab_pack<true> : k_slab_pack<false>, dim3(L.blocks), dim3(SL_BLOCK), 0, st, P, cap, A.main_slots,
                       A.counting && A.overlap ? 1 : 0, O.lists ? 1 : 0, M.has_left, M.has_right, A.pos, A.vel, A.owned, A.out, A.hist, (uint2*)A.blockcnt,
                       L.stage_l, L.stage_r, A.counters, A.counter, A.key_s, O.prev_adv_lo, O.prev_adv_hi, O.skip_edge ? 1 : 0);
    if ((!L.hl && !L.hr) || !O.lists) return;                           // no neighbour / messages pre-built: nothing to send
    launch_slab_msg(st, P, A, M, L);
}
// words of `stage` and of the look-back state launch_slab_pack needs for `cap` slots
size_t slab_stage_words(uint32_t cap) { return 2 * (size_t)sl_blocks(cap) * SL_BLOCK; }
size_t slab_msg_groups(uint32_t cap) { return (sl_blocks(cap) + MSG_GROUP - 1u) / MSG_GROUP; }

void launch_slab_prepack(hipStream_t st, const StepParams& P_next, const SlabArrays& A, const SlabMessages& M, uint32_t edge_grid,
                         bool classify) {
    const MsgLayout L(A, M, A.cap);
    if (!L.hl && !L.hr) return;
    const bool walk = edge_grid != 0 && P_next.transposed;
    hipLaunchKernelGGL(k_slab_prepack, dim3(walk ? edge_grid : L.blocks), dim3(SL_BLOCK), 0, st, P_next, M.has_left, M.has_right, walk ? 1 : 0,
                       A.pos, A.vel, A.owned, A.key_s, A.cs, (uint2*)A.blockcnt, L.stage_l, L.stage_r, classify ? 1 : 0, A.counting ? 1 : 0, A.main_slots, A.out, A.hist, A.counters);
    launch_slab_msg(st, P_next, A, M, L, walk ? A.cs : nullptr, edge_grid);
}

void launch_slab_unpack(hipStream_t st, const StepParams& P, const SlabArrays& A, const SlabMessages& M) {
    const SlabHeader* hl = (const SlabHeader*)M.left;
    const SlabHeader* hr = (const SlabHeader*)M.right;
    hipLaunchKernelGGL(A.counting ? k_slab_unpack<true> : k_slab_unpack<false>, dim3(sl_blocks(2 * M.R)), dim3(SL_BLOCK), 0, st, P, A.main_slots, M.R,
                       hl, records(hl), hr, records(hr), A.pos_out, A.vel_out, A.out, A.hist, A.counters);
}

// bitonic slab mode only (the counting sort's k_cs_fixreorder<true> does the reorder itself)
void launch_slab_reorder(hipStream_t st, const StepParams& P, const SlabArrays& A, uint32_t work_cap) {
    hipLaunchKernelGGL(k_slab_reorder, dim3(sl_blocks(A.cap)), dim3(SL_BLOCK), 0, st, P, A.cap, A.pairs, A.pos, A.vel, A.pos_s,
                       A.vel_s, A.pred, A.key_s, A.owned, A.cs, A.start_ref, (GapEntry*)A.work, A.counter, work_cap, A.counters, A.safe, A.fdefer, A.fcount);
    launch_fill_gaps(st, A.cs, A.work, A.counter, work_cap);
}

void launch_slab_export(hipStream_t st, const StepParams& P, const SlabArrays& A) {
    hipLaunchKernelGGL(k_slab_export, dim3(sl_blocks(A.cap)), dim3(SL_BLOCK), 0, st, P, A.cap, A.pos, A.pred, A.vel, A.rho, A.key_s, (AosParticle*)A.aos);
}

void launch_slab_import(hipStream_t st, const StepParams& P, const SlabArrays& A, uint32_t n) {
    hipLaunchKernelGGL(k_slab_import, dim3(sl_blocks(A.cap)), dim3(SL_BLOCK), 0, st, P, n, A.cap, (const AosParticle*)A.aos, A.pos_out,
                       A.pred, A.vel_out, A.rho, A.key_s, A.owned);
}

void launch_slab_colhist(hipStream_t st, const StepParams& P, const SlabArrays& A, uint32_t* hist_global, uint32_t migr_count) {
    hipLaunchKernelGGL(k_slab_colhist, dim3(sl_blocks(P.grid_w)), dim3(SL_BLOCK), 0, st, P, A.cs, hist_global);
    if (migr_count)
        hipLaunchKernelGGL(k_slab_colhist_migrants, dim3(sl_blocks(migr_count)), dim3(SL_BLOCK), 0, st, P, A.main_slots, migr_count, A.owned, A.key_s, hist_global);
}

size_t slab_message_bytes(uint32_t R) { return sizeof(SlabHeader) + (size_t)R * sizeof(float4); }

}  // namespace fsd
