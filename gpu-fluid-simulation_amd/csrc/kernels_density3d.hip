// kernels_density3d.hip — the density pass of the 3D step and, beside it, the opt-in colour-field pass of the surface tension
// (DESIGN.md §19), with their launchers (fs_3d.h).  Both are ONE walk over the planes of the 27-cell sweep (fs_sweep3.h),
// PlaneTerms3, with their own terms: DensityPass computes the pass masks and hands them over, TensionPass fetches them.
// Rows in order 0, 1, 2, candidates ascending = the oracle's visiting order, so sums are bit-identical.
#include <hip/hip_runtime.h>

#include "fs_sweep3.h"

namespace fsd {

__device__ __forceinline__ float dens3(const Params3& P, float4 me, float4 q) {
    const float dx = q.x - me.x, dy = q.y - me.y, dz = q.z - me.z;
    const float r2 = dx * dx + dy * dy + dz * dz;
    float kern = 0.0f;
    if (!(r2 > P.h2)) { const float d = P.h2 - r2; kern = P.poly6 * d * d * d; }
    return P.mass * kern * 1.0f;
}

__device__ __forceinline__ float dens3_tol(const Params3& P, float4 me, float4 q, float acc) {
    const float dx = q.x - me.x, dy = q.y - me.y, dz = q.z - me.z;
    const float r2 = __builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, dz * dz));
    const float t = fmaxf(P.h2 - r2, 0.0f);                               // NaN candidate: contributes nothing
    return __builtin_fmaf(t * t, t, acc);
}

// The density terms of the set bits of one pass mask, ascending (bit 63 - t = candidate base[t]).
template <int MODE>
__device__ __forceinline__ void walk_density(const Params3& P, u64m mask, const float4* base, float4 me, float& rho) {
    while (mask) {
        const uint32_t t = (uint32_t)__builtin_clzll(mask);
        mask ^= 0x8000000000000000ull >> t;
        if (MODE == 2) rho = dens3_tol(P, me, base[t], rho); else rho += dens3(P, me, base[t]);
    }
}

// The density terms as PlaneTerms3 takes them.  Waves whose rows fit the masks scan the plane into masks, store them
// (Params3::handoff) and add the terms of the set bits (the candidates outside the radius contribute +0 in the oracle: no bit of a
// non-negative sum changes); other waves loop over their candidates.  MODE 2 (FS_MATH_TOLERANCE): FMA terms, the constant once.
template <int MODE>
struct DensityPass {
    const Params3& P;
    const Lane3& L;
    u64m* __restrict__ masks;
    float rho;
    __device__ __forceinline__ float4 staged(float4 c) const { return c; }
    __device__ __forceinline__ void plane_masks(int plane, const RowRanges& R, const uint32_t* blo, const float4* s_flat, u64m m[3], uint32_t la[3]) {
        scan3_plane(P, R, blo, L.me, s_flat, m, la);
        if (P.handoff && L.live) {
#pragma unroll
            for (int r = 0; r < 3; ++r) masks[mask3_slot(P, 0, plane, r, L.i)] = m[r];
        }
    }
    __device__ __forceinline__ void row_masks(int plane, int r, const float4* base, uint32_t len, u64m* mh, u64m* ml) {
        scan3_row128(P, base, len, L.me, mh, ml);
        if (P.handoff && L.live) {
            masks[mask3_slot(P, 0, plane, r, L.i)] = *mh;
            masks[mask3_slot(P, 1, plane, r, L.i)] = *ml;
        }
    }
    __device__ __forceinline__ void walk(u64m mask, const float4* base) { walk_density<MODE>(P, mask, base, L.me, rho); }
    __device__ __forceinline__ void one(float4 c) { if (MODE == 2) rho = dens3_tol(P, L.me, c, rho); else rho += dens3(P, L.me, c); }
    __device__ __forceinline__ void row(const float4* sp, uint32_t k, uint32_t hi) {      // staged candidates sp[k .. hi)
        const float4 me = L.me;
        if (MODE == 2) { for (; k < hi; ++k) rho = dens3_tol(P, me, sp[k], rho); return; }
        for (; k + 4u <= hi; k += 4u) {
            const float t0 = dens3(P, me, sp[k]), t1 = dens3(P, me, sp[k + 1u]);
            const float t2 = dens3(P, me, sp[k + 2u]), t3 = dens3(P, me, sp[k + 3u]);
            rho += t0; rho += t1; rho += t2; rho += t3;
        }
        for (; k < hi; ++k) rho += dens3(P, me, sp[k]);
    }
};

// ---- opt-in surface tension (include/fluidsim.h "3D surface tension") ---------------------------------
// The colour-field pass: per sorted slot i, over the neighbours k3_density visits (i itself included, same order),
//     n += w_j * (((Cg d) d) o),   L += w_j * ((Cg d) (7 r2 - 3 h2)),   o = q_j - q_i, d = h2 - r2, w_j = m / rho_j
// then st = ((-sigma L) / |n|) n where |n| > tau and |n| > 0, else 0.  k3_density's walk with another term.  A staged candidate
// is {q.xyz, w}: the division happens once per staged candidate, a neighbour costs one 16-byte LDS read.
struct TensionAcc { float nx, ny, nz, L; };
__device__ __forceinline__ void tension_add(const Tension3& T, float4 me, float4 c, TensionAcc& A) {    // c = {q_j.xyz, w_j}, in radius
    const float ox = c.x - me.x, oy = c.y - me.y, oz = c.z - me.z;
    const float r2 = ox * ox + oy * oy + oz * oz;
    const float d = T.h2 - r2;
    const float k = (T.cg * d) * d;
    A.nx += c.w * (k * ox); A.ny += c.w * (k * oy); A.nz += c.w * (k * oz);
    const float lk = (T.cg * d) * ((7.0f * r2) - T.h2x3);
    A.L += c.w * lk;
}
// One candidate of the sweeps without masks: the radius test of dens3 first.
__device__ __forceinline__ void tension_try(const Tension3& T, float4 me, float4 c, TensionAcc& A) {
    const float ox = c.x - me.x, oy = c.y - me.y, oz = c.z - me.z;
    const float r2 = ox * ox + oy * oy + oz * oz;
    if (!(r2 > T.h2)) tension_add(T, me, c, A);
}
// The terms of the set bits of one pass mask, ascending (bit 63 - t = candidate base[t]); the next candidate's read is issued
// before this one's terms (walk_density is scheduled differently on purpose).
__device__ __forceinline__ void walk_tension(const Tension3& T, u64m mask, const float4* base, float4 me, TensionAcc& A) {
    float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    bool have = mask != 0ull;
    if (have) { const uint32_t t = (uint32_t)__builtin_clzll(mask); mask ^= 0x8000000000000000ull >> t; c = base[t]; }
    while (have) {
        const float4 c0 = c;
        have = mask != 0ull;
        if (have) { const uint32_t t = (uint32_t)__builtin_clzll(mask); mask ^= 0x8000000000000000ull >> t; c = base[t]; }
        tension_add(T, me, c0, A);
    }
}

// The tension terms as PlaneTerms3 takes them: k3_density's walk with another term and — handed over — the same pass masks.
struct TensionPass {
    const Params3& P;
    const Tension3& T;
    const Lane3& L;
    const u64m* __restrict__ masks;
    TensionAcc A;
    __device__ __forceinline__ float4 staged(float4 c) const { c.w = __fdiv_rn(P.mass, c.w); return c; }   // w_j
    __device__ __forceinline__ void plane_masks(int plane, const RowRanges& R, const uint32_t* blo, const float4* s_flat, u64m m[3], uint32_t la[3]) {
        masks3_plane(P, masks, plane, L.ii, R, blo, L.me, s_flat, m, la);
    }
    __device__ __forceinline__ void row_masks(int plane, int r, const float4* base, uint32_t len, u64m* mh, u64m* ml) {
        masks3_row128(P, masks, plane, r, L.ii, base, len, L.me, mh, ml);
    }
    __device__ __forceinline__ void walk(u64m mask, const float4* base) { walk_tension(T, mask, base, L.me, A); }
    __device__ __forceinline__ void one(float4 c) { tension_try(T, L.me, c, A); }
    __device__ __forceinline__ void row(const float4* sp, uint32_t k, uint32_t hi) { for (; k < hi; ++k) tension_try(T, L.me, sp[k], A); }
};

// One plane of the sweep for a pass that adds per-neighbour terms, as sweep3_planes calls it: the workgroup's three row ranges
// staged into s_cand with coalesced loads — Terms::staged() once per staged candidate — then per wave: plane class 2, per row two
// mask words and their walks; class 1, three masks and their walks; class 0, a direct loop over the staged rows.  A plane that
// does not fit the tile: a direct loop on global memory, staged() per pair.
template <class Terms>
struct PlaneTerms3 {
    Terms& T;
    const float4* pred;
    float4* s_cand;
    __device__ __forceinline__ void operator()(int plane, const RowRanges& R, const uint32_t* blo, const uint32_t* bhi, bool fit, int pclass) const {
        if (fit) {
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma clang loop vectorize(disable)               // at most two trips (TILE3 candidates over B3F lanes)
                for (uint32_t j = threadIdx.x; j < bhi[r] - blo[r]; j += B3F) s_cand[r * TILE3_ROW + j] = T.staged(pred[blo[r] + j]);
            }
            __syncthreads();
            if (pclass == 2) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float4* base = s_cand + row_la(R, blo, r);
                    u64m mh, ml;
                    T.row_masks(plane, r, base, R.hi[r] - R.lo[r], &mh, &ml);
                    T.walk(mh, base);
                    T.walk(ml, base + 64);
                }
            } else if (pclass == 1) {
                u64m m[3];
                uint32_t la[3];
                T.plane_masks(plane, R, blo, s_cand, m, la);
#pragma unroll
                for (int r = 0; r < 3; ++r) T.walk(m[r], s_cand + la[r]);
            } else {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const bool any = R.lo[r] < R.hi[r];
                    T.row(s_cand + r * TILE3_ROW, any ? R.lo[r] - blo[r] : 0u, any ? R.hi[r] - blo[r] : 0u);
                }
            }
        } else {
#pragma unroll
            for (int r = 0; r < 3; ++r)
                for (uint32_t k = R.lo[r]; k < R.hi[r]; ++k) T.one(T.staged(pred[k]));
        }
    }
};

template <int MODE>
__global__ __launch_bounds__(B3F) void k3_density(Params3 P, float4* __restrict__ pred, const uint32_t* __restrict__ cs,
                                                 float4* __restrict__ vel_s, u64m* __restrict__ masks,
                                                 const uint32_t* __restrict__ key_s) {
    __shared__ float4 s_pred[TILE3_LDS + 64];   // a 128-candidate scan reads up to 131 entries from a range start
    __shared__ uint32_t s_red[24];
    Lane3 L;
    if (!sweep3_lane(P, pred, &L)) return;
    DensityPass<MODE> D{P, L, masks, 0.0f};
    sweep3_planes(P, cs, key_s, L, s_red, PlaneTerms3<DensityPass<MODE>>{D, pred, s_pred});
    if (!L.live) return;
    const uint32_t i = L.i; float rho = D.rho;
    if (MODE == 2) rho = rho * (P.mass * P.poly6);                 // sum of (h2 - r2)^3 -> density
    rho = fmaxf(rho, 1.19209290e-07f);
    rho = fmaxf(rho, 0.1f);
    reinterpret_cast<float*>(pred + i)[3] = rho;                   // pred.w <- density (other lanes read .xyz only)
    // vel_s.w <- +-RN(1/rho): what the force pass divides by, once per particle instead of once per pair; positive only
    // when every operand this particle brings to a pair is inside the proven quotient ranges (fs_device.h)
    float* yw = reinterpret_cast<float*>(vel_s + i) + 3;
    const float y = (P.share_div && rho <= FS_RCP_HI) ? rcp_rn_fast(rho) : __fdiv_rn(1.0f, rho);
    if (MODE == 2) { *yw = y; return; }                            // tolerance mode: no classification, the force pass has no exact quotients
    const bool ksafe = *yw > 0.0f;
    const float press = P.pressure_k * (rho - P.rest_density);     // the expression the force pass evaluates
    const bool ok = ksafe && rho <= FS_RCP_HI && fabsf(press) <= FS_PRESSURE_HI;
    *yw = ok ? y : -y;
}

__global__ __launch_bounds__(B3F) void k3_surface_tension(Params3 P, Tension3 T, const float4* __restrict__ pred,
                                                         const uint32_t* __restrict__ cs, const u64m* __restrict__ masks,
                                                         const uint32_t* __restrict__ key_s, float4* __restrict__ st) {
    __shared__ float4 s_cand[TILE3_LDS + 64];   // a 128-candidate scan reads up to 131 entries from a range start
    __shared__ uint32_t s_red[24];
    Lane3 L;
    if (!sweep3_lane(P, pred, &L)) return;
    TensionPass S{P, T, L, masks, {0.0f, 0.0f, 0.0f, 0.0f}};
    sweep3_planes(P, cs, key_s, L, s_red, PlaneTerms3<TensionPass>{S, pred, s_cand});
    if (!L.live) return;
    const TensionAcc& A = S.A;
    const float nl = sqrt_rn((A.nx * A.nx + A.ny * A.ny) + A.nz * A.nz);
    float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (nl > T.tau && nl > 0.0f) {
        const float sc = __fdiv_rn(-T.sigma * A.L, nl);
        f.x = sc * A.nx; f.y = sc * A.ny; f.z = sc * A.nz;
    }
    st[L.i] = f;
}

// ------------------------------------------------------------------------------------ launchers (fs_3d.h)
void launch3_density(hipStream_t st, const Params3& P, const Arrays3& A, bool tol) {
    const dim3 grid(xcd_grid3(blocks3(P.n), P.xcd_chunk_log2)), block(B3F);
    if (tol) hipLaunchKernelGGL(k3_density<2>, grid, block, 0, st, P, A.pred, A.cs, A.vel_s, A.masks, A.key);
    else hipLaunchKernelGGL(k3_density<0>, grid, block, 0, st, P, A.pred, A.cs, A.vel_s, A.masks, A.key);
}

// after launch3_density (pred.w, the masks), before launch3_force: writes st and nothing else
void launch3_surface_tension(hipStream_t stream, const Params3& P, const Arrays3& A, const Tension3& T, float4* st) {
    const dim3 grid(xcd_grid3(blocks3(P.n), P.xcd_chunk_log2)), block(B3F);
    hipLaunchKernelGGL(k3_surface_tension, grid, block, 0, stream, P, T, A.pred, A.cs, A.masks, A.key, st);
}

}  // namespace fsd
