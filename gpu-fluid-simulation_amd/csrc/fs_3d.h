// fs_3d.h — what the files of the 3D step share (kernels_3d.hip, kernels_density3d.hip, kernels_force3d.hip, kernels_bodies3d.hip: the kernels and
// their launchers, engine_3d*.hip over engine_3d.h: the handle and the fs3_* C ABI): the step parameters, the array set of the
// launchers, the launchers.  A header of its own:
// fs_kernels.h stays the 2D launchers' list, and kernels_sort_tile.inc takes the predict + cell-key expression from here.
#pragma once
#include "fs_count.h"
#include "fs_kernels.h"

namespace fsd {

struct Params3 {
    uint32_t n, gw, gh, gd, ncell;
    float dt, h, h2;
    float bx, by, bz;            // bounds * 0.5
    float mass, poly6, pressure_k, rest_density, damping, visc_coeff, spiky, visc_k;
    float gx, gy, gz;
    uint32_t frame;
    ConstDiv div_2h3, div_h2;    // exact constant divisions, proven at create (fs_device.h div_const)
    int32_t share_div;           // one reciprocal per denominator + div_by_rcp in the force pass (fs_device.h)
    int32_t handoff;             // k3_density stores its nine 64-bit pass masks per particle, k3_force walks them (no second scan)
    uint32_t xcd_chunk_log2;     // xcd_block3(): blocks per chunk dealt to one XCD
};

// The device arrays of a 3D handle as the launchers see them (fs_kernels.h StepArrays is the 2D form).  Host side only.
struct Arrays3 {
    float4* pos = nullptr;             // state before the step, source order (the order of the last step)
    float4* vel = nullptr;             // ... the force pass writes the new velocities over it
    float4* pos_out = nullptr;         // the spare position buffer: the force pass's new positions
    float4* vel_s = nullptr;           // sorted {vx, vy, vz, +-RN(1/rho)}: the sign is the particle's safe-operand classification
    float4* pred = nullptr;            // sorted predicted positions, .w = density; + FS_PRED_SLACK entries
    uint32_t* key = nullptr;           // sorted keys
    u64* pairs = nullptr;              // sorted (key << 32 | source slot)
    uint32_t* cs = nullptr;            // dense cell-start table, ncell + 1
    u64* masks = nullptr;              // 18 x n pass masks, k3_density -> k3_force (Params3::handoff), or nullptr
    void* work = nullptr;              // the gap worklist of the reorder pass ...
    uint32_t* counter = nullptr;       // ... and its counter
    uint32_t work_cap = 0;
    void* aos = nullptr;               // n fs3_particle records: import / export staging
};

// Predict + cell key of the 3D step, defined once for k3_predict_key, k3_reorder (kernels_3d.hip) and the sort's fused key
// generation (kernels_sort_tile.inc keygen3); the cell coordinates alone also for a query point (kernels_sample3d.hip).  K: anything with dt, h, bx, by, bz, gw, gh (Params3, KeyGen3).
template <class K>
__device__ __forceinline__ float4 predict3(const K& P, float4 p, float4 v) {
    float4 r;
    r.x = p.x + v.x * P.dt; r.y = p.y + v.y * P.dt; r.z = p.z + v.z * P.dt; r.w = 0.0f;
    if (fabsf(r.x) > P.bx) r.x = P.bx * sign_f32(r.x);
    if (fabsf(r.y) > P.by) r.y = P.by * sign_f32(r.y);
    if (fabsf(r.z) > P.bz) r.z = P.bz * sign_f32(r.z);
    return r;
}
template <class K>
__device__ __forceinline__ void cell_xyz3(const K& P, float4 pt, uint32_t* cx, uint32_t* cy, uint32_t* cz) {
    *cx = f32_to_u32_sat(floorf(__fdiv_rn(pt.x + P.bx, P.h))) + 1u;
    *cy = f32_to_u32_sat(floorf(__fdiv_rn(pt.y + P.by, P.h))) + 1u;
    *cz = f32_to_u32_sat(floorf(__fdiv_rn(pt.z + P.bz, P.h))) + 1u;
}
template <class K>
__device__ __forceinline__ uint32_t cell_key3(const K& P, float4 pt) {
    uint32_t cx, cy, cz;
    cell_xyz3(P, pt, &cx, &cy, &cz);
    return (cz * P.gh + cy) * P.gw + cx;
}

uint32_t blocks3(uint32_t n);          // workgroups of the density / force kernels over n particles (before xcd_block3's padding)
void launch3_predict_key(hipStream_t st, const Params3& P, const Arrays3& A);   // FS3_SEPARATE_KEYGEN: else fused into the sort
void launch3_reorder(hipStream_t st, const Params3& P, const Arrays3& A);       // + launch_fill_gaps
void launch3_density(hipStream_t st, const Params3& P, const Arrays3& A, bool tol);
// The opt-in static collider of a handle (include/fluidsim.h "3D colliders") as the force pass's COLLIDE
// instantiations take it, by value and apart from Params3: one float4 push vector per voxel {x, y, z, 0}, voxel (i, j, k) at
// field[(k * h + j) * w + i], over the whole domain.  size: the settings' box, the divisor of the lookup.
struct Collide3 {
    const float4* field;
    uint32_t w, h, d;
    float sx, sy, sz;
};
// The opt-in surface tension of a handle (include/fluidsim.h "3D surface tension") as k3_surface_tension takes it,
// by value and apart from Params3: cg = 6.0f * poly6, h2x3 = 3.0f * h2 (one f32 multiply each, on the host).
struct Tension3 {
    float h2, cg, h2x3, sigma, tau;
};
// After launch3_density, before launch3_force: st[i] = {sx, sy, sz, 0} per sorted slot, from pred (.w = density), the cell table
// and — A.masks non-null — the pass masks k3_density handed over.
void launch3_surface_tension(hipStream_t st, const Params3& P, const Arrays3& A, const Tension3& T, float4* stf);
// Diffusion and buoyancy of the tracking channels (include/fluidsim.h "3D channel diffusion and buoyancy", DESIGN.md §28;
// kernels_diffuse3d.hip), after launch3_density and launch3_surface_tension, before launch3_force.  The plan of one step, by
// value: channel[0 .. count) are the diffusing channels, ascending, g[k] = (2 kappa) delta of channel[k]; buoyancy_channel >= 0:
// fb_out[i] = (st_in[i] +) (rho_i beta (reference - A_b[i])) gravity, .w = 0, which launch3_force takes as `stf`.  attr_in: the
// channels as the carry delivered them (channel c at c * stride); attr_out: the spare set, of which only the rows of the diffusing
// channels are written.  count == 0 and no buoyancy channel, or P.n == 0: no launch.
struct Diffuse3Plan {
    int count = 0;
    int channel[4] = {0, 0, 0, 0};
    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int buoyancy_channel = -1;
    float beta = 0.0f, reference = 0.0f, gravity_x = 0.0f, gravity_y = 0.0f, gravity_z = 0.0f;
};
void launch3_diffuse(hipStream_t st, const Params3& P, const Arrays3& A, const Diffuse3Plan D, const float* attr_in, float* attr_out,
                     uint32_t stride, const float4* st_in, float4* fb_out);
// done (may be null): signalled by the kernel's completion.  K (may be null: no collider, today's instantiations): the push
// operator runs in the kernel's tail, after the wall clamp.  stf (may be null: no surface tension, today's instantiations): the
// forces of launch3_surface_tension, added to the force sum.
void launch3_force(hipStream_t st, const Params3& P, const Arrays3& A, bool tol, hipEvent_t done, const Collide3* K = nullptr,
                   const float4* stf = nullptr);
// The opt-in moving bodies of a handle (include/fluidsim.h "3D moving bodies") as k3_bodies takes them, by value
// and apart from Params3 (kernels_bodies3d.hip).  Per body: the voxel field of Collide3 over the body's own box, and the motion
// of this enqueue.  r[3 * i + j]: row-major R, world = R * local.  body[0 .. count) are the slots in use, ascending.
constexpr uint32_t BODIES3_MAX = 8u;   // FS3_MAX_BODIES
struct Body3 {
    const float4* field;
    uint32_t w, h, d;
    float ex, ey, ez;            // the box's extent: the divisor of the lookup
    float hx, hy, hz;            // extent * 0.5f
    float cx, cy, cz;
    float r[9];
    float ux, uy, uz;
    float wx, wy, wz;
};
struct Bodies3 {
    uint32_t count;
    Body3 body[BODIES3_MAX];
};
// After launch3_force, on the positions (A.pos_out) and velocities (A.vel) it stored: the operators B of every body in order.
// P: n, bx, by, bz, damping.  done (may be null): signalled by the kernel's completion, as launch3_force's is.
void launch3_bodies(hipStream_t st, const Params3& P, const Arrays3& A, const Bodies3& B, hipEvent_t done);
// The same pass while the handle's loads are on (include/fluidsim.h "3D body loads"): k3_bodies_loads, which also
// adds each body's eight 64-bit words of this step (sum Q(j.xyz), sum Q(t.xyz), hits, dropped; by kernel index) into a row of
// `shards` (BODY_LOAD_SHARDS rows of BODY3_LOAD_ROW words, all zero on entry), then k3_body_loads_fold, which adds the rows into
// `words` (FS3_MAX_BODIES x 8, by slot: M.slot[kernel index]) and leaves `shards` zero again; the fold carries `done`.
constexpr uint32_t BODY3_LOAD_WORDS = 8u;
constexpr uint32_t BODY3_LOAD_ROW = BODIES3_MAX * BODY3_LOAD_WORDS;
static_assert(BODIES3_MAX == BODIES2_MAX, "BodyLoadMap (fs_kernels.h) holds a slot per body of either handle");
void launch3_bodies_loads(hipStream_t st, const Params3& P, const Arrays3& A, const Bodies3& B, const BodyLoadMap& M,
                          unsigned long long* shards, unsigned long long* words, hipEvent_t done);
void launch3_import(hipStream_t st, uint32_t n, const Arrays3& A);   // aos -> pos, pred, vel, key
void launch3_export(hipStream_t st, uint32_t n, const Arrays3& A);   // ... and back

// 3D field sampling (kernels_sample3d.hip): n queries against pred (.w = density), vel and cs as the last step
// left them.  P: n, gw, gh, gd, h, h2, bx, by, bz, mass, poly6.  Device pointers; host side only.
struct Sample3Query {
    uint32_t n = 0;                    // points, or width * height * depth
    const float* points = nullptr;     // n fs_vec3, or nullptr: the voxel centres of the view below
    float3 wmin{}, wmax{};
    uint32_t width = 0, height = 0, depth = 0;
    void* out = nullptr;               // n fs3_sample records
};
void launch3_sample(hipStream_t st, const Params3& P, const Arrays3& A, const Sample3Query& Q);

// The tracking channels at the same queries (kernels_sample_attr3d.hip): pred and cs of the same state, `channels`
// (1 .. FS_TRACK_MAX_CHANNELS) arrays of n floats in slot order, channel c at attr + c * attr_stride.
struct Sample3AttrQuery {
    uint32_t n = 0;                    // points, or width * height * depth
    const float* points = nullptr;     // n fs_vec3, or nullptr: the voxel centres of the view below
    float3 wmin{}, wmax{};
    uint32_t width = 0, height = 0, depth = 0;
    int channels = 0;
    const float* attr = nullptr;
    uint32_t attr_stride = 0;
    float* weight_out = nullptr;       // n floats, or nullptr
    float* attr_out = nullptr;         // channel c at attr_out + c * n
};
void launch3_sample_attr(hipStream_t st, const Params3& P, const Arrays3& A, const Sample3AttrQuery& Q);

// 3D surface rendering (kernels_render3d.hip): one ray per pixel of a width x height image, marched against the
// same state and the same P as a Sample3Query.  Passed to the kernel by value.
struct Surface3Query {
    float3 eye{}, forward{}, right{}, up{};
    uint32_t width = 0, height = 0;
    int32_t orthographic = 0;
    float iso = 0.0f, t_near = 0.0f, ds = 0.0f;
    uint32_t max_steps = 0, refine = 0;
    void* out = nullptr;               // width * height fs3_surface_hit records, device
};
void launch3_render_surface(hipStream_t st, const Params3& P, const Arrays3& A, const Surface3Query& Q);

// 3D surface extraction (kernels_mesh3d.hip): surface nets over the node lattice of a view, against the same state
// and the same P as a Sample3Query.  Device pointers; host side only.  The scratch belongs to the handle: `field` and `rank` hold
// width * height * depth entries, `sums` two words per workgroup (mesh3_workgroups).
struct Mesh3Query {
    float3 wmin{}, wmax{};
    uint32_t width = 0, height = 0, depth = 0;   // nodes per axis, each >= 2, product <= 2^26
    float iso = 0.0f;
    float* field = nullptr;            // node densities
    uint32_t* rank = nullptr;          // vertex index of the cell whose low corner the node is (active cells only)
    uint32_t* sums = nullptr;          // per workgroup {vertices, quads}: counts, then exclusive offsets
    uint32_t* counts = nullptr;        // {V, T}
    void* verts = nullptr;             // vert_cap fs3_mesh_vertex records (may be null when vert_cap == 0)
    uint32_t vert_cap = 0;
    uint32_t* tris = nullptr;          // 3 * tri_cap indices (may be null when tri_cap == 0)
    uint32_t tri_cap = 0;
};
uint32_t mesh3_workgroups(uint32_t nodes);
void launch3_mesh_count(hipStream_t st, const Params3& P, const Arrays3& A, const Mesh3Query& Q);   // field, flags, offsets -> counts
void launch3_mesh_verts(hipStream_t st, const Params3& P, const Arrays3& A, const Mesh3Query& Q);   // after _count: rank, verts[0, vert_cap)
void launch3_mesh_faces(hipStream_t st, const Mesh3Query& Q);                                       // after _verts: tris[0, tri_cap)


// 3D collider producer (kernels_collide3d.hip): a w x h x d u8 mask (> 128: solid) to the push field of Collide3 by
// an exact Euclidean distance transform in index space, three separable u32 passes.  Device pointers; host side only.  `near_x` and
// `near_xy` hold w * h * d words each (the nearest free voxel after the X pass, packed x | y << 16 after the Y pass).
constexpr uint32_t COLLIDER3_MAX_EXTENT = 1024u;   // the largest extent: the host's check and the LDS line of the three passes
struct ColliderMask3 {
    const uint8_t* mask = nullptr;
    uint32_t w = 0, h = 0, d = 0;      // each 1 .. COLLIDER3_MAX_EXTENT
    float vx = 0.0f, vy = 0.0f, vz = 0.0f;   // voxel edge per axis: size.a / (float)W_a
    uint32_t* near_x = nullptr;
    uint32_t* near_xy = nullptr;
    float4* field = nullptr;           // out
};
void launch3_collider_from_mask(hipStream_t st, const ColliderMask3& Q);

// 3D fluid diagnostics (kernels_stats3d.hip): k3_stats over the arrays launch3_export reads (pred.w: the density),
// one row of stats_words(3) words per block into `slab`, then the fold of fs_kernels.h into the 232-byte fs3_stats record at `out`.
struct Stats3Input {
    uint32_t n = 0;
    const float4* pos = nullptr;
    const float4* vel = nullptr;
    const float4* pred = nullptr;
    int channels = 0;
    const float* attr = nullptr;       // channel c at attr + c * attr_stride
    uint32_t attr_stride = 0;
    uint32_t tick = 0;
};
void launch3_stats(hipStream_t st, const Stats3Input& I, unsigned long long* slab, void* out);

// A particle count that changes at run time: fs_count.h, for both handles.

}  // namespace fsd
