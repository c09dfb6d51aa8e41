// fs_force_sweep.h — the two neighbour sweeps of the 2D force kernels (kernels_force.hip): force_sweep_masks, the common
// case (staged rows of at most 32 candidates), and force_sweep_chunks, everything else (dense clusters).  Both scan a row's
// candidates into pass bits and then walk the set bits; what a hit costs is in fs_force_pair.h.
#pragma once
#include "fs_force_pair.h"
#include "fs_neighbours.h"

namespace fsd {

// ---------------------------------------------------------- force + integrate
// Two phases per lane so the expensive body (pressure + viscosity terms of one in-radius neighbour)
// runs with dense lanes:
//   scan  - test `k != i && !(r2 > sqr_radius)` (compute.wgsl:195,202) for the candidates of the three
//           row ranges and record the outcome as pass bits in registers (no branches, no lists);
//   heavy - every lane walks its set bits in the reference visiting order, so sums keep their association.
// force_sweep_masks handles the common case (all three rows of every lane of the wave <= 32 candidates:
// three masks, walked without idle lanes), force_sweep_chunks everything else.

// k_force stages the predicted positions of its three sweep rows in LDS: NBF_TILE candidates per row plus
// NBF_PAD of slack (the mask scans read up to 32 entries from a range start, whatever the range's length).
// Velocity and {density, 1/density} of the few in-radius neighbours are gathered in the heavy phase instead
// (staging them too cost occupancy and measured slower).
#define NBF_PAD 32u
#define NBF_ROW (NBF_TILE + NBF_PAD)     // LDS row pitch

// ---- chunked sweep: the general case (a row range of the wave is longer than 32, or the rows do not
// fit the LDS tile: dense clusters).  Same machinery as the mask sweep below, one 32-candidate chunk of
// one row at a time: wave-uniform scan of the chunk into a register mask (v_cmp + v_addc_co per
// candidate), then every lane walks its set bits.  Rows and chunks are taken in order, so a lane still
// visits its neighbours in the reference order; lanes idle while others finish a chunk (dense regions
// only — the common case never comes here).  STAGED: candidates from the LDS tile, else from global
// memory (the pred array is allocated with FS_PRED_SLACK elements of slack for the read-ahead).
template <bool STAGED, int MODE>
__device__ __forceinline__ void force_sweep_chunks(const StepParams& P, const RowRanges& R, const uint32_t* blo,
                                                   uint32_t ii, const float2 me, const float2 mv, float pressure,
                                                   const float2* __restrict__ pred, const float2* __restrict__ vel_s,
                                                   const float2* __restrict__ rho2, const float2* s_flat, bool me_ok,
                                                   ForceAcc& A) {
    const float lim = P.sqr_radius;
    constexpr bool FAST = MODE == 1;
    const TolConsts TC = tol_consts(P);
    const wave_mask me_okm = wm(me_ok);      // the lane's own "safe operand" classification (all lanes active here)
    // plain registers: as arrays the row selects below become dynamic indexing, which the compiler
    // serves from scratch / promoted LDS
    uint32_t lo0 = R.lo[0], lo1 = R.lo[1], lo2 = R.lo[2], hi0 = R.hi[0], hi1 = R.hi[1], hi2 = R.hi[2];
    uint32_t b00 = blo[0], b01 = blo[1], b02 = blo[2];
    asm volatile("" : "+v"(lo0), "+v"(lo1), "+v"(lo2), "+v"(hi0), "+v"(hi1), "+v"(hi2), "+v"(b00), "+v"(b01), "+v"(b02));
#pragma unroll 1
    for (int r = 0; r < 3; ++r) {
        const uint32_t lo = r == 0 ? lo0 : r == 1 ? lo1 : lo2;
        const uint32_t hi = r == 0 ? hi0 : r == 1 ? hi1 : hi2;
        const uint32_t b0 = r == 0 ? b00 : r == 1 ? b01 : b02;
        const uint32_t len = hi - lo;
        // Round 3: FS_CHUNK_BATCH chunks of 32 candidates are scanned before the walk starts, and their masks are walked as
        // ONE shift register (cur <- n1 <- n2 <- n3; the chunks of a batch are consecutive in the row, so a refill only
        // advances the two bases by 32 candidates).  With one chunk per walk a lane waited for the wave's slowest lane after
        // every ~11 hits (lane utilisation 0.66 in the dense regime, profiles/r03_counters_2d_dense.md); over 128
        // candidates the hit counts of the lanes differ relatively less.
#ifndef FS_CHUNK_BATCH
#define FS_CHUNK_BATCH 4
#endif
#pragma unroll 1
        for (uint32_t c0 = 0; __any(c0 < len); c0 += 32u * FS_CHUNK_BATCH) {   // c0 is wave-uniform
            uint32_t mq[FS_CHUNK_BATCH];
            const uint32_t g0 = c0 < len ? lo + c0 : 0u;                  // global index of the batch's first candidate
            // byte offset of the batch's first candidate: into the LDS tile, or (32-bit, n <= 2^28) into pred
            const uint32_t boff0 = (STAGED ? (c0 < len ? (uint32_t)r * NBF_ROW + (g0 - b0) : 0u) : g0) << 3;
            const char* src = STAGED ? reinterpret_cast<const char*>(s_flat) : reinterpret_cast<const char*>(pred);
#define FS_CAND(off, k) (*reinterpret_cast<const float2*>(src + ((off) + ((k) << 3))))
#pragma unroll
            for (int q = 0; q < FS_CHUNK_BATCH; ++q) {
                const uint32_t cq = c0 + 32u * (uint32_t)q;
                const uint32_t clen = cq < len ? (len - cq < 32u ? len - cq : 32u) : 0u;
                const uint32_t boff = clen ? boff0 + 256u * (uint32_t)q : 0u;
                uint32_t mask = 0, t = 0;
                if (__any(0u < clen)) do {              // tested at the bottom, as in force_sweep_masks
                    const float2 q0 = FS_CAND(boff, t), q1 = FS_CAND(boff, t + 1u), q2 = FS_CAND(boff, t + 2u), q3 = FS_CAND(boff, t + 3u);
                    const float2 qq[4] = {q0, q1, q2, q3};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float ox = qq[u].x - me.x, oyv = qq[u].y - me.y;
                        shift_in_not_greater(mask, ox * ox + oyv * oyv, lim);
                    }
                    t += 4u;
                } while (__any(t < clen));
                mask = t ? mask << (32u - t) : 0u;
                mask &= clen ? 0xFFFFFFFFu << (32u - clen) : 0u;
                const uint32_t g = g0 + 32u * (uint32_t)q;
                if (r == 1 && clen && ii - g < clen) mask &= ~(0x80000000u >> (ii - g));   // k != i
                mq[q] = mask;
            }
            // walk, software-pipelined by one neighbour; (boff, goff) are the bases of the chunk `cur` belongs to
            uint32_t cur = mq[0], n1 = FS_CHUNK_BATCH > 1 ? mq[1 % FS_CHUNK_BATCH] : 0u, n2 = FS_CHUNK_BATCH > 2 ? mq[2 % FS_CHUNK_BATCH] : 0u,
                     n3 = FS_CHUNK_BATCH > 3 ? mq[3 % FS_CHUNK_BATCH] : 0u;
            uint32_t boff = boff0, goff = g0 << 3;
            float2 qn = make_float2(0.0f, 0.0f), vn = qn, dn = qn;
            bool have = false, pending = false;
#define FS_FETCH_NEXT1()                                                                                             \
    do {                                                                                                             \
        if (cur == 0u) { cur = n1; n1 = n2; n2 = n3; n3 = 0u; boff += 256u; goff += 256u; }   /* next chunk of the batch */ \
        have = cur != 0u;                                                                                            \
        pending = (cur | n1 | n2 | n3) != 0u;            /* an empty chunk in the middle costs this lane one idle trip */ \
        if (have) {                                                                                                  \
            const uint32_t t8 = (uint32_t)__builtin_clz(cur) << 3;                                                   \
            cur ^= 0x80000000u >> (t8 >> 3);                                                                         \
            qn = FS_CAND(boff, t8 >> 3);                                                                             \
            const uint32_t off = goff + t8;                                                                          \
            vn = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(vel_s) + off);                       \
            dn = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(rho2) + off);                        \
        }                                                                                                            \
    } while (0)
            FS_FETCH_NEXT1();
            wave_mask pendm = wm(pending);              // the loop test on the scalar unit, as in force_sweep_masks
            while (pendm != 0) {
                const bool cur_valid = have;
                const float2 q0 = qn, v0 = vn, d0 = dn;
                FS_FETCH_NEXT1();
                pendm = wm(pending);
                if (cur_valid && MODE == 2) {
                    force_accum_tol(P, TC, me, mv, pressure, q0, v0, d0, A);
                } else if (cur_valid) {
                    ForceTerms T0;
                    if (FAST) {
                        T0 = force_terms<true>(P, me, mv, pressure, q0, v0, d0.x, A.seed);
                    } else {
                        wave_mask good = 0;
                        if (P.share_div) { T0 = force_terms_shared(P, me, mv, pressure, q0, v0, d0, good); good &= me_okm; }
                        if (good != wm(true)) {
                            T0 = force_terms<false>(P, me, mv, pressure, q0, v0, d0.x, A.seed);
                        }
                    }
                    A.fpx += T0.px; A.fpy += T0.py; A.fvx += T0.vx; A.fvy += T0.vy;
                }
            }
#undef FS_FETCH_NEXT1
#undef FS_CAND
        }
    }
}

// ---- mask sweep: the normal case (staged tiles, no row range of the wave longer than 32) ----------
//   scan  — per sweep row one 32-bit pass mask in a register.  Per candidate: the LDS read, r2, and
//           v_cmp_ngt + v_addc_co, which shifts `!(r2 > sqr_radius)` (compute.wgsl:202; true for NaN
//           like the shader's test) into the mask — no branch, no LDS write.  Trip counts are
//           wave-uniform (longest range of the wave, in fours); a lane masks off what lies past its
//           own range afterwards, and the middle row clears the lane's own bit (`k != i`, :195).
//   heavy — every lane walks its set bits, row 0, 1, 2, ascending = the reference visiting order, so
//           the sums keep their association; all lanes stay busy until the longest list is done.
// GENERAL = false (the lean main kernel): a pair whose operands fall outside the proven ranges is not re-evaluated
// here — the wave remembers it (`bad`) and the caller hands the whole wave to the general kernel instead, so the
// exact true-division body never enters this kernel's register allocation.
template <int MODE, bool GENERAL>
__device__ __forceinline__ bool force_sweep_masks(const StepParams& P, const RowRanges& R, const uint32_t* blo,
                                                  uint32_t ii, const float2 me, const float2 mv, float pressure,
                                                  const float2* __restrict__ vel_s, const float2* __restrict__ rho2,
                                                  const float2* s_flat /* [3][NBF_ROW] */, bool me_ok, ForceAcc& A) {
    uint32_t m[3], la[3];                    // masks (bit 31-t <=> candidate lo+t), flat LDS index of lo
    const float lim = P.sqr_radius;
    constexpr bool FAST = MODE == 1;
    const TolConsts TC = tol_consts(P);
    bool bad = false;                        // wave-uniform
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const uint32_t len = R.hi[r] - R.lo[r];                           // <= 32 (caller)
        la[r] = (uint32_t)r * NBF_ROW + (len ? R.lo[r] - blo[r] : 0u);
        const float2* base = s_flat + la[r];
        uint32_t mask = 0, t = 0;
        // t is wave-uniform.  Tested at the bottom: with the test on top the mask is copied out of and back into the register the
        // asm operand is tied to on every trip (two v_mov of 32 issue slots)
        if (__any(0u < len)) do {
            const float2 q0 = base[t], q1 = base[t + 1u], q2 = base[t + 2u], q3 = base[t + 3u];
            const float2 qq[4] = {q0, q1, q2, q3};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float ox = qq[u].x - me.x, oyv = qq[u].y - me.y;
                shift_in_not_greater(mask, ox * ox + oyv * oyv, lim);
            }
            t += 4u;
        } while (__any(t < len));
        // candidate t sits at bit (trips - 1 - t): left-align, keep the lane's own len candidates
        mask = t ? mask << (32u - t) : 0u;
        mask &= len ? 0xFFFFFFFFu << (32u - len) : 0u;
        if (r == 1 && ii - R.lo[1] < len) mask &= ~(0x80000000u >> (ii - R.lo[1]));
        m[r] = mask;
    }
    // The three masks are walked as a shift register (round 3): `cur` is the mask being consumed with its LDS / global
    // bases, (n1, n2) wait behind it.  Empty masks are squeezed out first, so "cur == 0 -> pull n1" is all a refill ever
    // needs, and the per-neighbour bit extraction touches ONE mask and ONE pair of bases instead of selecting among three
    // masks and six bases.  Row order 0, 1, 2 (= the reference visiting order) is kept.
    // Software-pipelined: the LDS read and the two gathers of a later neighbour are issued before the terms of
    // neighbour k are evaluated, so a lane's own arithmetic covers their latency.  FS_PIPE_DEPTH = 1: neighbour
    // k+1 (one slot, rotated by moves); 2: neighbours k+1 and k+2 (three slots A, B, C refilled in turn, the loop
    // unrolled by three so no value is moved).
    const wave_mask me_okm = wm(me_ok);      // the lane's own "safe operand" classification (all lanes active here)
    uint32_t cur = m[0], n1 = m[1], n2 = m[2];
    uint32_t lac = la[0] << 3, la_1 = la[1] << 3, la_2 = la[2] << 3, loc = R.lo[0] << 3, lo_1 = R.lo[1] << 3, lo_2 = R.lo[2] << 3;   // bytes
    if (n1 == 0u) { n1 = n2; la_1 = la_2; lo_1 = lo_2; n2 = 0u; }
    if (cur == 0u) { cur = n1; lac = la_1; loc = lo_1; n1 = n2; la_1 = la_2; lo_1 = lo_2; n2 = 0u; }
#define FS_FETCH(have, qn, vn, dn)                                                                                   \
    do {                                                                                                             \
        have = cur != 0u;                                                                                            \
        if (have) {                                                                                                  \
            const uint32_t t8 = (uint32_t)__builtin_clz(cur) << 3;                                                   \
            cur ^= 0x80000000u >> (t8 >> 3);                                                                         \
            qn = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(s_flat) + (lac + t8));               \
            /* both arrays hold 8-B elements: one 32-bit byte offset from the two SGPR bases (n <= 2^28) */          \
            const uint32_t off = loc + t8;                                                                           \
            vn = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(vel_s) + off);                       \
            dn = *reinterpret_cast<const float2*>(reinterpret_cast<const char*>(rho2) + off); /* {rho, 1/rho} */     \
            if (cur == 0u) { cur = n1; lac = la_1; loc = lo_1; n1 = n2; la_1 = la_2; lo_1 = lo_2; n2 = 0u; }         \
        }                                                                                                            \
    } while (0)
#define FS_PAIR(cur_valid, q0, v0, d0)                                                                               \
    do {                                                                                                             \
        if (cur_valid && MODE == 2) {                                                                                \
            force_accum_tol(P, TC, me, mv, pressure, q0, v0, d0, A);                                                 \
        } else if (cur_valid) {                                                                                      \
            ForceTerms T0;                                                                                           \
            if (FAST) {                                                                                              \
                T0 = force_terms<true>(P, me, mv, pressure, q0, v0, d0.x, A.seed);                                   \
            } else {                                                                                                 \
                wave_mask good = 0;                                                                                  \
                if (P.share_div) { T0 = force_terms_shared(P, me, mv, pressure, q0, v0, d0, good); good &= me_okm; } \
                if (good != wm(true)) {             /* rare, wave-uniform */                                         \
                    if (GENERAL) T0 = force_terms<false>(P, me, mv, pressure, q0, v0, d0.x, A.seed);                 \
                    else bad = true;                                                                                 \
                }                                                                                                    \
            }                                                                                                        \
            A.fpx += T0.px; A.fpy += T0.py; A.fvx += T0.vx; A.fvy += T0.vy;                                          \
        }                                                                                                            \
    } while (0)
    // measured at 16M: depth 2 is worth 2.3 % to the strict kernel (0.721 -> 0.705 ms) and COSTS the tolerance-mode
    // kernel 5 % (0.57 -> 0.60 ms: with 24 instructions per pair the extra selects and registers outweigh the cover)
    if constexpr (MODE == 2) {
    float2 qn = make_float2(0.0f, 0.0f), vn = qn, dn = qn;
    bool have = false;
    FS_FETCH(have, qn, vn, dn);
    // "does any lane still hold a neighbour" as the ballot of the compare that formed `have`, tested on the scalar unit: through
    // __any() the flag took a v_cndmask and a v_cmp per neighbour to reach the branch
    wave_mask havem = wm(have);
    while (havem != 0) {
        const bool cur_valid = have;
        const float2 q0 = qn, v0 = vn, d0 = dn;
        FS_FETCH(have, qn, vn, dn);
        havem = wm(have);
        FS_PAIR(cur_valid, q0, v0, d0);
    }
    } else {
    float2 qA = make_float2(0.0f, 0.0f), vA = qA, dA = qA, qB = qA, vB = qA, dB = qA, qC = qA, vC = qA, dC = qA;
    bool hA = false, hB = false, hC = false;
    FS_FETCH(hA, qA, vA, dA);
    FS_FETCH(hB, qB, vB, dB);
    FS_FETCH(hC, qC, vC, dC);
    // A slot is refilled right after its neighbour's terms: two bodies later it is consumed.  The queue only drains, so an empty
    // slot means the slots fetched after it are empty too: the loop has ONE exit (on A).  In the last trip B and C may be empty
    // for the whole wave: their terms are skipped on the empty exec mask and their fetches find the queue empty again.  (With
    // an exit in front of every body the accumulators were copied for the exits, three v_mov per neighbour.)
    wave_mask mA = wm(hA);                   // the ballot of hA, for the scalar unit (see the loop above)
    while (mA != 0) {
        { const bool cv = hA; const float2 q0 = qA, v0 = vA, d0 = dA; FS_PAIR(cv, q0, v0, d0); }
        mA = wm(cur != 0u);                  // the hA of the fetch below (taken in front of it: behind it costs two v_mov a trip)
        FS_FETCH(hA, qA, vA, dA);
        { const bool cv = hB; const float2 q0 = qB, v0 = vB, d0 = dB; FS_PAIR(cv, q0, v0, d0); }
        FS_FETCH(hB, qB, vB, dB);
        { const bool cv = hC; const float2 q0 = qC, v0 = vC, d0 = dC; FS_PAIR(cv, q0, v0, d0); }
        FS_FETCH(hC, qC, vC, dC);
    }
    }
#undef FS_PAIR
#undef FS_FETCH
    // `bad` was set under the exec mask of the lanes that were evaluating the failing pair: make it the wave's
    return __any(bad);
}

}  // namespace fsd
