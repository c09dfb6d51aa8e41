// kernels_diffuse3d.hip — opt-in diffusion and buoyancy of the tracking channels of the 3D step, between the
// density pass (and the surface-tension pass, when on) and the force pass; the 3D counterpart of kernels_diffuse.hip.
//   k3_diffuse<D> = D diffusing channels (1 or 2) over the density pass's neighbour walk; its tail also forms the buoyancy force
//   k3_buoyancy   = the buoyancy force alone (no diffusing channel): no walk
//
// Normative statement: include/fluidsim.h "3D channel diffusion and buoyancy".  Per sorted slot i, over the candidates the density
// pass visits (27 cells, z outer, the particle itself included), all f32 without contraction:
//   o = q_j - q_i, r2 = o.o;  skip if r2 > h2;  d = h2 - r2;  w = m / rho_j;  wk = w * ((Cg d) d)
//   acc_c += wk * (A_c[j] - A_c[i])                       for each diffusing channel c
// then u_i = 1 / rho_i and A_c'[i] = A_c[i] + (g_c acc_c) u_i with g_c = (2 kappa_c) delta from the host.  Jacobi: every A_c[j] is
// read from `attr_in` and every A_c' goes to the same row of `attr_out`, the spare tracking set; a channel that does not diffuse
// is neither read nor written.
// The walk is k3_surface_tension's (fs_sweep3.h: sweep3_lane, sweep3_planes, plane_class, the pass masks k3_density handed over).
// PlaneTerms3 (kernels_density3d.hip) hands its terms a candidate's VALUE; here a candidate is its staged record {q.xyz, w} plus D
// channel values in float arrays of the same pitch beside the rows, so the plane body below, DiffusePlane3, hands on indices.
// LDS: 21 472 B + D x 5 344 B.
// Buoyancy (channel b, one of the diffusing ones or not): a = A_b[i] before the pass,
//   s = beta (A0 - a);  rs = rho_i s;  fb = (st_i +) (rs g.x, rs g.y, rs g.z), fb.w = 0
// which launch3_force takes as its `stf` operand.
#include <hip/hip_runtime.h>

#include "fs_sweep3.h"

namespace fsd {

// By value: the diffusing channels of this launch and the buoyancy channel's constants.
struct Diffuse3Consts {
    float h2, cg;
    uint32_t ch[2];                 // channel index of each of the D accumulators, ascending
    float g[2];                     // (2 kappa_c) delta of each
    int32_t buoy;                   // the buoyancy channel, or -1: this launch writes no fb
    float beta, a0, gx, gy, gz;
};

template <int D> struct Df3Val { float v[D]; };

// One candidate c = {q_j.xyz, w_j} with channel values a.  TEST: the radius test of the sweeps without masks, by a select, not a
// product with zero (a skipped candidate's A may be a NaN).  An accumulator that starts at +0.0f is never -0.0f, so adding +0.0f
// for a skipped candidate IS skipping it.
template <int D, bool TEST>
__device__ __forceinline__ void df3_term(float h2, float cg, float4 me, const Df3Val<D>& mine, float4 c, const Df3Val<D>& a,
                                         Df3Val<D>& acc) {
    const float ox = c.x - me.x, oy = c.y - me.y, oz = c.z - me.z;
    const float r2 = ox * ox + oy * oy + oz * oz;
    const bool in = !TEST || !(r2 > h2);            // a NaN r2 is admitted (the statement's test, as written)
    const float d = h2 - r2;
    const float wk = c.w * ((cg * d) * d);
#pragma unroll
    for (int e = 0; e < D; ++e) acc.v[e] += in ? wk * (a.v[e] - mine.v[e]) : 0.0f;
}

// The buoyancy force of slot i (the tail of k3_diffuse, the whole of k3_buoyancy).
__device__ __forceinline__ float4 buoyancy3_force(const Diffuse3Consts& C, float a, float rho_i, const float4* __restrict__ st_in,
                                                  uint32_t i) {
    const float s = C.beta * (C.a0 - a);
    const float rs = rho_i * s;
    const float bx = rs * C.gx, by = rs * C.gy, bz = rs * C.gz;
    if (st_in) {
        const float4 f = st_in[i];
        return make_float4(f.x + bx, f.y + by, f.z + bz, 0.0f);
    }
    return make_float4(bx, by, bz, 0.0f);
}

// The diffusion terms of one lane: the staged plane (s_cand and, at the same index, s_a[e]) or global memory (pred, rows[e]).
template <int D>
struct DiffusePass3 {
    const Params3& P;
    const Diffuse3Consts& C;
    const Lane3& L;
    const u64m* __restrict__ masks;
    const float* const* rows;       // the D diffusing rows of attr_in
    const Df3Val<D>& mine;
    Df3Val<D>& acc;
    __device__ __forceinline__ float4 staged(float4 c) const { c.w = __fdiv_rn(P.mass, c.w); return c; }   // w_j
    __device__ __forceinline__ Df3Val<D> values(const float (*s_a)[TILE3_LDS + 64], uint32_t k) const {
        Df3Val<D> a;
#pragma unroll
        for (int e = 0; e < D; ++e) a.v[e] = s_a[e][k];
        return a;
    }
    // The terms of the set bits of one pass mask, ascending (bit 63 - t = candidate `at + t` of the stage); the next candidate's
    // reads are issued before this one's terms, as walk_tension does.
    __device__ __forceinline__ void walk(u64m mask, const float4* s_cand, const float (*s_a)[TILE3_LDS + 64], uint32_t at) {
        const float h2 = C.h2, cg = C.cg;
        float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        Df3Val<D> a{};
        bool have = mask != 0ull;
        if (have) {
            const uint32_t t = (uint32_t)__builtin_clzll(mask);
            mask ^= 0x8000000000000000ull >> t;
            c = s_cand[at + t]; a = values(s_a, at + t);
        }
        while (have) {
            const float4 c0 = c;
            const Df3Val<D> a0 = a;
            have = mask != 0ull;
            if (have) {
                const uint32_t t = (uint32_t)__builtin_clzll(mask);
                mask ^= 0x8000000000000000ull >> t;
                c = s_cand[at + t]; a = values(s_a, at + t);
            }
            df3_term<D, false>(h2, cg, L.me, mine, c0, a0, acc);
        }
    }
    // staged candidates [k, hi) of the stage, with the radius test
    __device__ __forceinline__ void row(const float4* s_cand, const float (*s_a)[TILE3_LDS + 64], uint32_t k, uint32_t hi) {
        const float h2 = C.h2, cg = C.cg;
        for (; k < hi; ++k) df3_term<D, true>(h2, cg, L.me, mine, s_cand[k], values(s_a, k), acc);
    }
    // candidate k of the sorted arrays, from global memory
    __device__ __forceinline__ void one(const float4* __restrict__ pred, uint32_t k) {
        Df3Val<D> a;
#pragma unroll
        for (int e = 0; e < D; ++e) a.v[e] = rows[e][k];
        df3_term<D, true>(C.h2, C.cg, L.me, mine, staged(pred[k]), a, acc);
    }
};

// One plane of the sweep, as sweep3_planes calls it — PlaneTerms3's shape (kernels_density3d.hip) with the channel arrays beside the
// rows: the workgroup's three row ranges staged with coalesced loads, the records as {q.xyz, w} into s_cand and the D channel
// values into s_a[e] at the same index, then per wave: plane class 2, per row two mask words and their walks; class 1, three
// masks and their walks; class 0, a loop over the staged rows with the radius test.  A plane that does not fit the tile: a
// loop on global memory.
template <int D>
struct DiffusePlane3 {
    DiffusePass3<D>& T;
    const float4* pred;
    float4* s_cand;
    float (*s_a)[TILE3_LDS + 64];
    __device__ __forceinline__ void operator()(int plane, const RowRanges& R, const uint32_t* blo, const uint32_t* bhi, bool fit, int pclass) const {
        if (fit) {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma clang loop vectorize(disable)               // at most two trips (TILE3 candidates over B3F lanes)
                for (uint32_t j = threadIdx.x; j < bhi[r] - blo[r]; j += B3F) {
                    s_cand[r * TILE3_ROW + j] = T.staged(pred[blo[r] + j]);
#pragma unroll
                    for (int e = 0; e < D; ++e) s_a[e][r * TILE3_ROW + j] = T.rows[e][blo[r] + j];
                }
            }
            __syncthreads();
            if (pclass == 2) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const uint32_t at = row_la(R, blo, r);
                    u64m mh, ml;
                    masks3_row128(T.P, T.masks, plane, r, T.L.ii, s_cand + at, R.hi[r] - R.lo[r], T.L.me, &mh, &ml);
                    T.walk(mh, s_cand, s_a, at);
                    T.walk(ml, s_cand, s_a, at + 64u);
                }
            } else if (pclass == 1) {
                u64m m[3];
                uint32_t la[3];
                masks3_plane(T.P, T.masks, plane, T.L.ii, R, blo, T.L.me, s_cand, m, la);
#pragma unroll
                for (int r = 0; r < 3; ++r) T.walk(m[r], s_cand, s_a, la[r]);
            } else {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const bool any = R.lo[r] < R.hi[r];
                    const uint32_t base = (uint32_t)r * TILE3_ROW;
                    T.row(s_cand, s_a, base + (any ? R.lo[r] - blo[r] : 0u), base + (any ? R.hi[r] - blo[r] : 0u));
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 3; ++r)
                for (uint32_t k = R.lo[r]; k < R.hi[r]; ++k) T.one(pred, k);
        }
    }
};

template <int D>
__global__ __launch_bounds__(B3F) void k3_diffuse(Params3 P, Diffuse3Consts C, const float4* __restrict__ pred,
                                                 const uint32_t* __restrict__ cs, const u64m* __restrict__ masks,
                                                 const uint32_t* __restrict__ key_s, const float* __restrict__ attr_in,
                                                 float* __restrict__ attr_out, uint32_t stride, const float4* __restrict__ st_in,
                                                 float4* __restrict__ fb_out) {
    __shared__ float4 s_cand[TILE3_LDS + 64];   // a 128-candidate scan reads up to 131 entries from a range start
    __shared__ float s_a[D][TILE3_LDS + 64];    // the candidates' channel values, same index
    __shared__ uint32_t s_red[24];
    Lane3 L;
    if (!sweep3_lane(P, pred, &L)) return;
    const float* rows[D];
    Df3Val<D> mine, acc;
#pragma unroll
    for (int e = 0; e < D; ++e) {               // the particle's own channel values: in flight with its record
        rows[e] = attr_in + (size_t)C.ch[e] * stride;
        mine.v[e] = rows[e][L.ii];
        acc.v[e] = 0.0f;
    }
    DiffusePass3<D> S{P, C, L, masks, rows, mine, acc};
    sweep3_planes(P, cs, key_s, L, s_red, DiffusePlane3<D>{S, pred, s_cand, s_a});
    if (!L.live) return;
    const uint32_t i = L.i;
    const float rho_i = L.me.w;
    const float u = __fdiv_rn(1.0f, rho_i);
#pragma unroll
    for (int e = 0; e < D; ++e) attr_out[(size_t)C.ch[e] * stride + i] = mine.v[e] + (C.g[e] * acc.v[e]) * u;
    if (C.buoy >= 0)            // uniform
        fb_out[i] = buoyancy3_force(C, attr_in[(size_t)C.buoy * stride + i], rho_i, st_in, i);
}

__global__ __launch_bounds__(B3F) void k3_buoyancy(uint32_t n, Diffuse3Consts C, const float4* __restrict__ pred,
                                                  const float* __restrict__ attr_in, uint32_t stride,
                                                  const float4* __restrict__ st_in, float4* __restrict__ fb_out) {
    const uint32_t i = blockIdx.x * B3F + threadIdx.x;
    if (i >= n) return;
    const float rho_i = reinterpret_cast<const float*>(pred + i)[3];
    fb_out[i] = buoyancy3_force(C, attr_in[(size_t)C.buoy * stride + i], rho_i, st_in, i);
}

namespace {
Diffuse3Consts consts_of(const Params3& P, const Diffuse3Plan& D, int first, int d, bool with_buoyancy) {
    Diffuse3Consts C{};
    C.h2 = P.h2;
    C.cg = 6.0f * P.poly6;          // Tension3::cg
    for (int k = 0; k < d; ++k) { C.ch[k] = (uint32_t)D.channel[first + k]; C.g[k] = D.g[first + k]; }
    C.buoy = with_buoyancy ? D.buoyancy_channel : -1;
    C.beta = D.beta; C.a0 = D.reference; C.gx = D.gravity_x; C.gy = D.gravity_y; C.gz = D.gravity_z;
    return C;
}
}  // namespace

void launch3_diffuse(hipStream_t stream, const Params3& P, const Arrays3& A, const Diffuse3Plan D, const float* attr_in, float* attr_out,
                     uint32_t stride, const float4* st_in, float4* fb_out) {
    if (P.n == 0) return;
    const bool buoy = D.buoyancy_channel >= 0;
    const dim3 block(B3F);
    if (D.count == 0) {
        if (!buoy) return;
        hipLaunchKernelGGL(k3_buoyancy, dim3(blocks3(P.n)), block, 0, stream, P.n, consts_of(P, D, 0, 0, true), A.pred, attr_in, stride,
                           st_in, fb_out);
        return;
    }
    // Launches of two channels plus a last one of one when the count is odd (channels are independent under Jacobi semantics: the
    // same bits under any grouping); the buoyancy tail rides the first launch.
    const dim3 grid(xcd_grid3(blocks3(P.n), P.xcd_chunk_log2));
    for (int first = 0; first < D.count; first += 2) {
        const int d = D.count - first >= 2 ? 2 : 1;
        const Diffuse3Consts C = consts_of(P, D, first, d, buoy && first == 0);
        if (d == 2) hipLaunchKernelGGL(k3_diffuse<2>, grid, block, 0, stream, P, C, A.pred, A.cs, A.masks, A.key, attr_in, attr_out, stride, st_in, fb_out);
        else hipLaunchKernelGGL(k3_diffuse<1>, grid, block, 0, stream, P, C, A.pred, A.cs, A.masks, A.key, attr_in, attr_out, stride, st_in, fb_out);
    }
}

}  // namespace fsd
