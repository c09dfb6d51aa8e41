// kernels_mesh3d.hip — 3D surface extraction (build extension): the iso-surface of the 3D fluid's density as an
// indexed triangle mesh, by surface nets: one vertex per lattice cell the surface crosses, one quad per interior lattice edge it
// crosses.  Reads the cell-sorted state the last step left on the device (pred with the density in .w, vel, cs) through the
// walks of fs_field3.h.  No reference counterpart (the reference is 2D only).
//
// Statement (include/fluidsim.h "3D surface extraction"), f32 without contraction, / and sqrt correctly rounded:
//   node (i, j, k) = fs3_sample_grid's voxel centre;  F = density(node);  inside = F >= iso
//   cell (i, j, k), corners (i+a, j+b, k+c): active when its corners are neither all inside nor all outside
//   vertex of an active cell: over its twelve edges (four x-, four y-, four z-edges, each at (0,0), (1,0), (0,1), (1,1) of the
//     other two axes) every crossing adds tt = (iso - Fa) / (Fb - Fa) along the edge's axis and its corner offsets along the
//     others;  l.a = s_a / (float)c;  position.a = N_a(i_a) + l.a * (N_a(i_a + 1) - N_a(i_a));  S = sample(position)
//   quad of an interior lattice edge whose ends differ: the vertices of the four cells around it, wound by the low node's side
//   vertex order: ascending cell index;  quad order: ascending 3 * node + axis
//
// Passes, all stream-ordered launches, nothing waits on another workgroup:
//   k3_mesh_field  one lane per node, a wave is a 4 x 4 x 4 node tile (a workgroup 8 x 8 x 4), the density-only walk
//   k3_mesh_count  one lane per node in LINEAR order (the output order), as the low corner of its cell and the low end of its
//                  three edges: eight corner values -> active flag, three face flags; per-workgroup sums of both
//   k3_mesh_scan   ONE workgroup over the <= 2^18 workgroup sums: sums -> exclusive offsets, totals -> counts
//   k3_mesh_verts  the flags again, a workgroup scan -> the cell's rank (stored per node for the faces), the vertex, one full sample
//   k3_mesh_faces  the flags again, a workgroup scan -> the quad's rank; the four cells' ranks give six indices
// Every output position is a prefix sum of flags in the statement's order: no atomics anywhere.
#include "fs_field3.h"
#include "fs_scan.h"      // block_scan3

namespace fsd {

struct MeshVertex3 {               // fs3_mesh_vertex (include/fluidsim.h), 40 bytes
    float px, py, pz, nx, ny, nz, vx, vy, vz, density;
};
static_assert(sizeof(MeshVertex3) == 40, "fs3_mesh_vertex is 40 bytes");

#define B3M 256                    // workgroup of every pass but the scan: four waves
#define B3M_SCAN 1024              // the scan's single workgroup

struct Lattice3 {                  // by value: the view, the node count (<= 2^26) and the threshold
    float3 wmin, wmax;
    uint32_t w, h, d, n;
    float iso;
};

// N_a(i): fs3_sample_grid's voxel centre along one axis (k3_sample's expression).
__device__ __forceinline__ float node_coord3(float lo, float hi, uint32_t i, uint32_t ext) {
    return lo + __fdiv_rn((float)i + 0.5f, (float)ext) * (hi - lo);
}

__global__ __launch_bounds__(B3M) void k3_mesh_field(Params3 P, Lattice3 L, uint32_t nbx, uint32_t nby,
                                                          const float4* __restrict__ pred, const uint32_t* __restrict__ cs,
                                                          float* __restrict__ field) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t bi = blockIdx.x % nbx, bj = (blockIdx.x / nbx) % nby, bk = blockIdx.x / (nbx * nby);
    const uint32_t i = (bi << 3) + ((wave & 1u) << 2) + (lane & 3u);
    const uint32_t j = (bj << 3) + ((wave >> 1) << 2) + ((lane >> 2) & 3u);
    const uint32_t k = (bk << 2) + (lane >> 4);
    if (i >= L.w || j >= L.h || k >= L.d) return;                   // edge tiles are masked
    const float x = node_coord3(L.wmin.x, L.wmax.x, i, L.w);
    const float y = node_coord3(L.wmin.y, L.wmax.y, j, L.h);
    const float z = node_coord3(L.wmin.z, L.wmax.z, k, L.d);
    field[(k * L.h + j) * L.w + i] = density3_at(P, x, y, z, pred, cs);     // < n <= 2^26
}

// What node q is as the low corner of its cell and the low end of its three edges.  0 when q is no node or has no cell: an
// interior edge has its u- and v-coordinates <= extent - 2 and its own <= extent - 2, so its low node always has a cell.
//   bit 0: the cell is active;  bits 1..3: the x-, y-, z-edge from q emits a quad;  bit 4: q is inside;  bits 8..15: the corners'
//   inside bits, corner (a, b, c) at bit a + 2 b + 4 c.  f[8]: the corner values (set when the cell exists).
__device__ __forceinline__ uint32_t node_flags3(const Lattice3& L, const float* __restrict__ field, uint32_t q, uint32_t* i,
                                                uint32_t* j, uint32_t* k, float f[8]) {
    if (q >= L.n) return 0u;
    const uint32_t r = q / L.w;
    *i = q - r * L.w; *j = r % L.h; *k = r / L.h;
    if (*i + 1u >= L.w || *j + 1u >= L.h || *k + 1u >= L.d) return 0u;
    const uint32_t sy = L.w, sz = L.w * L.h;
    uint32_t mask = 0u;
#pragma unroll
    for (uint32_t c = 0u; c < 8u; ++c) {                            // q + 1 + sy + sz is node (i+1, j+1, k+1) < n
        f[c] = field[q + (c & 1u) + ((c >> 1) & 1u) * sy + (c >> 2) * sz];
        mask |= (f[c] >= L.iso ? 1u : 0u) << c;
    }
    const uint32_t in0 = mask & 1u;
    uint32_t flags = (mask != 0u && mask != 255u) ? 1u : 0u;
    if (*j >= 1u && *k >= 1u && ((mask >> 1) & 1u) != in0) flags |= 2u;
    if (*k >= 1u && *i >= 1u && ((mask >> 2) & 1u) != in0) flags |= 4u;
    if (*i >= 1u && *j >= 1u && ((mask >> 4) & 1u) != in0) flags |= 8u;
    return flags | (in0 << 4) | (mask << 8);
}

// vertices in the low half, quads in the high half: a workgroup holds at most 256 and 768
__device__ __forceinline__ uint32_t packed_counts3(uint32_t flags) { return (flags & 1u) | ((uint32_t)__popc((flags >> 1) & 7u) << 16); }

__global__ __launch_bounds__(B3M) void k3_mesh_count(Lattice3 L, const float* __restrict__ field, uint2* __restrict__ sums) {
    __shared__ uint32_t s_wave[B3M / 64];
    uint32_t i, j, k, total;
    float f[8];
    const uint32_t flags = node_flags3(L, field, blockIdx.x * B3M + threadIdx.x, &i, &j, &k, f);
    (void)block_scan3<B3M / 64>(packed_counts3(flags), s_wave, &total);
    if (threadIdx.x == 0u) sums[blockIdx.x] = make_uint2(total & 0xFFFFu, total >> 16);
}

// One workgroup: thread t owns the sums [t * chunk, (t + 1) * chunk) (chunk <= 256).  In place: sums -> exclusive offsets.
// counts[0] = V, counts[1] = T = 2 * quads (<= 6 * 2^26).
__global__ __launch_bounds__(B3M_SCAN) void k3_mesh_scan(uint32_t nwg, uint32_t chunk, uint2* __restrict__ sums,
                                                              uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_v[B3M_SCAN / 64], s_q[B3M_SCAN / 64];
    const uint32_t lo = threadIdx.x * chunk < nwg ? threadIdx.x * chunk : nwg;
    const uint32_t hi = lo + chunk < nwg ? lo + chunk : nwg;
    uint32_t v = 0u, qd = 0u;
    for (uint32_t b = lo; b < hi; ++b) { const uint2 s = sums[b]; v += s.x; qd += s.y; }
    uint32_t tv, tq;
    uint32_t ev = block_scan3<B3M_SCAN / 64>(v, s_v, &tv);
    uint32_t eq = block_scan3<B3M_SCAN / 64>(qd, s_q, &tq);
    for (uint32_t b = lo; b < hi; ++b) {
        const uint2 s = sums[b];
        sums[b] = make_uint2(ev, eq);
        ev += s.x; eq += s.y;
    }
    if (threadIdx.x == 0u) { counts[0] = tv; counts[1] = 2u * tq; }
}

__global__ __launch_bounds__(B3M) void k3_mesh_verts(Params3 P, Lattice3 L, const float* __restrict__ field,
                                                          const uint2* __restrict__ sums, const float4* __restrict__ pred,
                                                          const float4* __restrict__ vel, const uint32_t* __restrict__ cs,
                                                          uint32_t* __restrict__ rank, MeshVertex3* __restrict__ verts,
                                                          uint32_t vert_cap) {
    __shared__ uint32_t s_wave[B3M / 64];
    const uint32_t q = blockIdx.x * B3M + threadIdx.x;
    uint32_t i, j, k, total;
    float f[8];
    const uint32_t flags = node_flags3(L, field, q, &i, &j, &k, f);
    const uint32_t excl = block_scan3<B3M / 64>(packed_counts3(flags), s_wave, &total);
    if (!(flags & 1u)) return;
    const uint32_t r = sums[blockIdx.x].x + (excl & 0xFFFFu);
    rank[q] = r;                                                    // q < n: the cell's low corner
    if (r >= vert_cap) return;
    const uint32_t mask = flags >> 8;
    const float iso = L.iso;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    uint32_t c = 0u;
#pragma unroll
    for (uint32_t e = 0u; e < 4u; ++e) {                            // x-edges at (y0, z0) = (e & 1, e >> 1)
        const uint32_t a = 2u * (e & 1u) + 4u * (e >> 1);
        if (((mask >> a) ^ (mask >> (a + 1u))) & 1u) {
            sx += __fdiv_rn(iso - f[a], f[a + 1u] - f[a]); sy += (float)(e & 1u); sz += (float)(e >> 1); c += 1u;
        }
    }
#pragma unroll
    for (uint32_t e = 0u; e < 4u; ++e) {                            // y-edges at (x0, z0)
        const uint32_t a = (e & 1u) + 4u * (e >> 1);
        if (((mask >> a) ^ (mask >> (a + 2u))) & 1u) {
            sy += __fdiv_rn(iso - f[a], f[a + 2u] - f[a]); sx += (float)(e & 1u); sz += (float)(e >> 1); c += 1u;
        }
    }
#pragma unroll
    for (uint32_t e = 0u; e < 4u; ++e) {                            // z-edges at (x0, y0)
        const uint32_t a = (e & 1u) + 2u * (e >> 1);
        if (((mask >> a) ^ (mask >> (a + 4u))) & 1u) {
            sz += __fdiv_rn(iso - f[a], f[a + 4u] - f[a]); sx += (float)(e & 1u); sy += (float)(e >> 1); c += 1u;
        }
    }
    const float fc = (float)c;                                      // an active cell has c >= 3
    const float lx = __fdiv_rn(sx, fc), ly = __fdiv_rn(sy, fc), lz = __fdiv_rn(sz, fc);
    const float x0 = node_coord3(L.wmin.x, L.wmax.x, i, L.w), x1 = node_coord3(L.wmin.x, L.wmax.x, i + 1u, L.w);
    const float y0 = node_coord3(L.wmin.y, L.wmax.y, j, L.h), y1 = node_coord3(L.wmin.y, L.wmax.y, j + 1u, L.h);
    const float z0 = node_coord3(L.wmin.z, L.wmax.z, k, L.d), z1 = node_coord3(L.wmin.z, L.wmax.z, k + 1u, L.d);
    MeshVertex3 o;
    o.px = x0 + lx * (x1 - x0); o.py = y0 + ly * (y1 - y0); o.pz = z0 + lz * (z1 - z0);
    const FullSample3 S = sample3_at(P, o.px, o.py, o.pz, pred, vel, cs);
    const float gl = sqrt_rn((S.gx * S.gx + S.gy * S.gy) + S.gz * S.gz);
    o.nx = 0.0f; o.ny = 0.0f; o.nz = 0.0f; o.vx = 0.0f; o.vy = 0.0f; o.vz = 0.0f;
    if (gl > 0.0f) { o.nx = __fdiv_rn(-S.gx, gl); o.ny = __fdiv_rn(-S.gy, gl); o.nz = __fdiv_rn(-S.gz, gl); }
    if (S.weight > 0.0f) { o.vx = __fdiv_rn(S.vx, S.weight); o.vy = __fdiv_rn(S.vy, S.weight); o.vz = __fdiv_rn(S.vz, S.weight); }
    o.density = S.density;
    verts[r] = o;                                                   // r < vert_cap
}

__global__ __launch_bounds__(B3M) void k3_mesh_faces(Lattice3 L, const float* __restrict__ field, const uint2* __restrict__ sums,
                                                          const uint32_t* __restrict__ rank, uint32_t* __restrict__ tris,
                                                          uint32_t tri_cap) {
    __shared__ uint32_t s_wave[B3M / 64];
    const uint32_t q = blockIdx.x * B3M + threadIdx.x;
    uint32_t i, j, k, total;
    float f[8];
    const uint32_t flags = node_flags3(L, field, q, &i, &j, &k, f);
    const uint32_t excl = block_scan3<B3M / 64>(packed_counts3(flags), s_wave, &total);
    if (!(flags & 14u)) return;
    uint32_t qr = sums[blockIdx.x].y + (excl >> 16);
    const uint32_t stride[3] = {1u, L.w, L.w * L.h};
#pragma unroll
    for (uint32_t A = 0u; A < 3u; ++A) {
        if (!(flags & (2u << A))) continue;
        // the edge is interior: its u- and v-coordinates are >= 1, so the three cells below q exist (and are active: each holds the edge)
        const uint32_t su = stride[(A + 1u) % 3u], sv = stride[(A + 2u) % 3u];
        const uint32_t a = rank[q - su - sv], b = rank[q - sv], c = rank[q], d = rank[q - su];
        const bool low_inside = (flags & 16u) != 0u;
        const uint32_t v1 = low_inside ? b : d, v3 = low_inside ? d : b;
        const uint32_t t0 = 2u * qr;                                // < 6 * 2^26; 3 * t0 + 5 < 2^31
        if (t0 < tri_cap) { tris[3u * t0] = a; tris[3u * t0 + 1u] = v1; tris[3u * t0 + 2u] = c; }
        if (t0 + 1u < tri_cap) { tris[3u * t0 + 3u] = a; tris[3u * t0 + 4u] = c; tris[3u * t0 + 5u] = v3; }
        qr += 1u;
    }
}

static Lattice3 lattice_of(const Mesh3Query& Q) {
    Lattice3 L;
    L.wmin = Q.wmin; L.wmax = Q.wmax;
    L.w = Q.width; L.h = Q.height; L.d = Q.depth; L.n = Q.width * Q.height * Q.depth;
    L.iso = Q.iso;
    return L;
}

uint32_t mesh3_workgroups(uint32_t nodes) { return (nodes + B3M - 1u) / B3M; }

void launch3_mesh_count(hipStream_t st, const Params3& P, const Arrays3& A, const Mesh3Query& Q) {
    const Lattice3 L = lattice_of(Q);
    const uint32_t nbx = (L.w + 7u) >> 3, nby = (L.h + 7u) >> 3, nbz = (L.d + 3u) >> 2;      // <= 16 n / 256 = 2^22 workgroups
    const uint32_t nwg = mesh3_workgroups(L.n);
    hipLaunchKernelGGL(k3_mesh_field, dim3(nbx * nby * nbz), dim3(B3M), 0, st, P, L, nbx, nby, A.pred, A.cs, Q.field);
    hipLaunchKernelGGL(k3_mesh_count, dim3(nwg), dim3(B3M), 0, st, L, Q.field, (uint2*)Q.sums);
    hipLaunchKernelGGL(k3_mesh_scan, dim3(1), dim3(B3M_SCAN), 0, st, nwg, (nwg + B3M_SCAN - 1u) / B3M_SCAN, (uint2*)Q.sums, Q.counts);
}

void launch3_mesh_verts(hipStream_t st, const Params3& P, const Arrays3& A, const Mesh3Query& Q) {
    const Lattice3 L = lattice_of(Q);
    hipLaunchKernelGGL(k3_mesh_verts, dim3(mesh3_workgroups(L.n)), dim3(B3M), 0, st, P, L, Q.field, (const uint2*)Q.sums, A.pred,
                       A.vel, A.cs, Q.rank, (MeshVertex3*)Q.verts, Q.vert_cap);
}

void launch3_mesh_faces(hipStream_t st, const Mesh3Query& Q) {
    const Lattice3 L = lattice_of(Q);
    hipLaunchKernelGGL(k3_mesh_faces, dim3(mesh3_workgroups(L.n)), dim3(B3M), 0, st, L, Q.field, (const uint2*)Q.sums, Q.rank,
                       Q.tris, Q.tri_cap);
}

}  // namespace fsd
