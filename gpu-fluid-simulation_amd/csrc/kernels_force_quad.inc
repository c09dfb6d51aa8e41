// kernels_force_quad.inc — k_force_quad, the force kernel for a SHORT list of deferred waves (four lanes per particle),
// and its quad helpers.  A fragment of kernels_force.hip, included there behind the kernels whose integrate_store,
// block_may_advance and parameter list (FS_FORCE_ARGS) it uses; launched by launch_force.
// (FS_QSELECT and FS_QROUND are macros on purpose: as functions — a slot struct, or reference parameters — the same
// statements cost k_force_quad<0, true, *> two VGPRs and with them a wave per SIMD, 97 against 95.)

// ---- k_force_quad: a SHORT pre-registered list, four lanes per particle (round 4; VERDICT r3 item 4) -------------------------
// The general kernel's time on a short list — a small scene, a slab rank, the first dense clusters of any scene — is the
// latency of ONE wave: 64 particles of 60 - 70 in-radius neighbours each, ~11 000 instructions at the single-wave issue rate
// (40 us per step at 1 M particles, profiles/r04_rejected.md), with most of the chip idle.  Here a deferred wave's 64
// particles are spread over a whole 256-thread workgroup, FOUR LANES PER PARTICLE: the quad scans the particle's candidates
// 64 at a time (16 each), ORs the hits into one 64-bit mask in candidate order, and walks it four neighbours per round — lane
// l evaluates the l-th set bit — after which the four terms are added to the (replicated) sums in lane order by quad
// broadcasts: neighbour order and association are exactly the reference's.  (A lane without a neighbour contributes +0.0f:
// the sums start at +0.0f and a round-to-nearest sum is never -0.0f unless both addends are, so x + 0.0f == x bit for bit.)
// Shared-reciprocal terms only (strict math), native forms (FS_MATH_WGSL_ULP); a pair outside the proven ranges — or a
// coincident pair, whose direction comes from the particle's serial random sequence — sends the wave to the late list, which
// k_force_general takes afterwards.  Candidates are read from global memory: no tile, any row length.
__device__ __forceinline__ uint32_t quad_or(uint32_t x) {
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1 /* quad_perm [1, 0, 3, 2] */, 0xf, 0xf, true);
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E /* quad_perm [2, 3, 0, 1] */, 0xf, 0xf, true);
    return x;
}
template <int K> __device__ __forceinline__ float quad_lane(float x) {      // the value lane K of the quad holds
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), K * 0x55, 0xf, 0xf, true));
}
__device__ __forceinline__ void mask64_clear_top(uint32_t& hi, uint32_t& lo) {
    const uint32_t t = hi ? hi : lo;
    const uint32_t bit = t ? 0x80000000u >> __builtin_clz(t) : 0u;
    if (hi) hi ^= bit; else lo ^= bit;
}
template <int MODE, bool AOS, bool ST>
__global__ __launch_bounds__(FS_BLOCK) void k_force_quad(FS_FORCE_ARGS, uint32_t* __restrict__ hint, const float2* __restrict__ st_in) {
    constexpr bool FAST = MODE == 1;
    const uint32_t n = P.n_live ? *P.n_live : P.n;
    const uint32_t count = work_count[FS_LIST_PRE];                // written by k_density earlier in the stream
    if (hint && blockIdx.x == 0 && threadIdx.x == 0) *hint = count + work_count[FS_LIST_LATE];
    const uint32_t tid = threadIdx.x, l = tid & 3u;
    const float lim = P.sqr_radius;
    const uint32_t lbit = 0x80000000u >> l;             // candidate 4 t + l of a chunk: bit 31 - (4 t + l) of its half
    // consecutive work items to workgroups far apart in dispatch order (fs_force_lists.h)
    for (uint32_t item = force_list_spread(); item < 4u * count; item += gridDim.x) {
        const uint32_t blk = worklist[item >> 2], w = item & 3u;
        if (!((defer_bits[force_defer_word(blk, FS_LIST_PRE)] >> w) & 1u)) continue;           // uniform: this wave of the block was not deferred
        if (!block_may_advance(P, pairs, blk, n)) continue;          // uniform
        const uint32_t i = blk * FS_BLOCK + w * 64u + (tid >> 2);
        bool live = i < n;
        const uint32_t ii = live ? i : n - 1u;
        const uint32_t lo_fix = quirk_lo_fix(P, pairs, cs, start_ref);
        const float2 me = pred[ii];
        const float2 mv = vel_s[ii];
        const float2 mrec = rho2[ii];
        const float2 p_own = pos_s[P.pos_by_src ? (uint32_t)pairs[ii] : ii];
        const float mrho = mrec.x;
        const float pressure = P.pressure_k * (mrho - P.rest_density);
        ForceAcc A;
        A.fpx = A.fpy = A.fvx = A.fvy = 0.0f;
        A.seed = 0u;                                      // never drawn from here
        uint32_t cx, cy;
        int32_t cg;
        uv_local(P, me, &cx, &cy, &cg);
        if (P.n_live && !slab_advances(P, cg)) live = false;
        bool bad = live && !FAST && !(mrec.y > 0.0f);     // the particle's own operands are outside the proven ranges
        const wave_mask allm = wm(true);
        // one row at a time (its range lives only as long as its sweep), not lane_row_ranges: no tile, no block-wide bounds here
#pragma unroll 1
        for (int r = 0; r < 3; ++r) {
            uint32_t lo = 0, hi = 0;
            if (live) (void)row_range(P, cs, cx, cy + (uint32_t)(r - 1), lo_fix, &lo, &hi);
            const uint32_t len = hi > lo ? hi - lo : 0u;
#pragma unroll 1
            for (uint32_t c0 = 0; __any(c0 < len); c0 += 64u) {
                // scan: this lane's sixteen candidates of the chunk, c0 + 4 t + l
                uint32_t Mh = 0, Ml = 0;
                {   // all sixteen loads in flight at once: in groups of four every group waited out a full round trip, and the
                    // round trips, not the arithmetic, were this kernel's time
                    float2 q[16];
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        const uint32_t c = c0 + 4u * (uint32_t)t + l;
                        q[t] = pred[c < len ? lo + c : ii];
                    }
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        const uint32_t c = c0 + 4u * (uint32_t)t + l;
                        const float ox = q[t].x - me.x, oyv = q[t].y - me.y;
                        const float r2 = ox * ox + oyv * oyv;
                        const bool hit = c < len && !(r2 > lim) && !(r == 1 && lo + c == ii);       // compute.wgsl:195,202
                        const uint32_t b = hit ? lbit >> (4 * (t & 7)) : 0u;
                        if (t < 8) Mh |= b; else Ml |= b;
                    }
                }
                Mh = quad_or(Mh); Ml = quad_or(Ml);       // the particle's hits in candidate order, in all four lanes
                const uint32_t jbase = lo + c0;
                // walk: four neighbours per round, lane l the l-th of them; two register sets, refilled in turn
#define FS_QSELECT(has, q, v, d)                                                                                     \
    do {                                                                                                             \
        uint32_t th = Mh, tl = Ml;                                                                                   \
        if (l > 0u) mask64_clear_top(th, tl);                                                                        \
        if (l > 1u) mask64_clear_top(th, tl);                                                                        \
        if (l > 2u) mask64_clear_top(th, tl);                                                                        \
        has = (th | tl) != 0u;                                                                                       \
        const uint32_t kk = th ? (uint32_t)__builtin_clz(th) : 32u + (uint32_t)__builtin_clz(tl | 1u);               \
        const uint32_t j = has ? jbase + kk : ii;                                                                    \
        q = pred[j]; v = vel_s[j]; d = rho2[j];                                                                      \
        mask64_clear_top(Mh, Ml); mask64_clear_top(Mh, Ml); mask64_clear_top(Mh, Ml); mask64_clear_top(Mh, Ml);      \
    } while (0)
#define FS_QROUND(has, q, v, d)                                                                                      \
    do {                                                                                                             \
        ForceTerms T0;                                                                                               \
        if (FAST) {                                                                                                  \
            const float ox = q.x - me.x, oyv = q.y - me.y;                                                           \
            if (has && ox * ox + oyv * oyv == 0.0f) bad = true;          /* coincident: the serial random direction */ \
            uint32_t seed = 0u;                                                                                      \
            T0 = force_terms<true>(P, me, mv, pressure, q, v, d.x, seed);                                            \
        } else {                                                                                                     \
            wave_mask good = 0;                                                                                      \
            T0 = force_terms_shared(P, me, mv, pressure, q, v, d, good);                                             \
            if ((good | ~wm(has)) != allm) bad = true;                   /* wave-uniform */                          \
        }                                                                                                            \
        if (!has) { T0.px = 0.0f; T0.py = 0.0f; T0.vx = 0.0f; T0.vy = 0.0f; }                                        \
        A.fpx += quad_lane<0>(T0.px); A.fpy += quad_lane<0>(T0.py); A.fvx += quad_lane<0>(T0.vx); A.fvy += quad_lane<0>(T0.vy); \
        A.fpx += quad_lane<1>(T0.px); A.fpy += quad_lane<1>(T0.py); A.fvx += quad_lane<1>(T0.vx); A.fvy += quad_lane<1>(T0.vy); \
        A.fpx += quad_lane<2>(T0.px); A.fpy += quad_lane<2>(T0.py); A.fvx += quad_lane<2>(T0.vx); A.fvy += quad_lane<2>(T0.vy); \
        A.fpx += quad_lane<3>(T0.px); A.fpy += quad_lane<3>(T0.py); A.fvx += quad_lane<3>(T0.vx); A.fvy += quad_lane<3>(T0.vy); \
    } while (0)
                bool hA = false, hB = false, hC = false;
                float2 qA, vA, dA, qB, vB, dB, qC, vC, dC;
                FS_QSELECT(hA, qA, vA, dA);
                FS_QSELECT(hB, qB, vB, dB);
                // two rounds' gathers in flight behind the one being evaluated; "does any lane hold a neighbour" as the ballot of
                // the compare that formed the flag, tested on the scalar unit (fs_force_sweep.h)
                wave_mask mA = wm(hA), mB = wm(hB), mC;
                for (;;) {
                    if (mA == 0) break;
                    FS_QSELECT(hC, qC, vC, dC); mC = wm(hC);
                    FS_QROUND(hA, qA, vA, dA);
                    if (mB == 0) break;
                    FS_QSELECT(hA, qA, vA, dA); mA = wm(hA);
                    FS_QROUND(hB, qB, vB, dB);
                    if (mC == 0) break;
                    FS_QSELECT(hB, qB, vB, dB); mB = wm(hB);
                    FS_QROUND(hC, qC, vC, dC);
                }
#undef FS_QROUND
#undef FS_QSELECT
            }
        }
        if (__syncthreads_or(bad ? 1 : 0)) {             // hand the whole wave to the late list, write nothing
            if (tid == 0) {
                force_list_push(defer_bits, worklist, work_count, P.n, blk, w, FS_LIST_LATE);
            }
            continue;
        }
        if (live && l == 0u)
            integrate_store<MODE, AOS, ST>(P, i, me, mv, mrec, mrho, p_own, A, cx, cy, tex, pos_out, vel_out, aos_out, rho_arr, st_in);
    }
}
