// row_ranges_checker.hip — TEST INFRASTRUCTURE, host only: lane_row_ranges (csrc/fs_neighbours.h, six loads issued together, selects
// afterwards) against three row_range calls (the form it replaced, which k_force_quad still uses) for EVERY input of small grids,
// the ones no particle of a single-domain handle can produce included: cx = 0, cy = 0, the wrapped cx - 1 and cy - 1 (coordinates
// 0xFFFFFFFF too), cy + 1 >= grid_v, id_lo past the table, id_hi clamped to ncell, dead lanes, a == 0 with every lo_fix, and tables
// that are not monotone (hi < lo).  Prints "cases N mismatches M"; exit status 1 on a mismatch.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fs_neighbours.h"

using namespace fsd;

static RowRanges three_calls(const StepParams& P, const uint32_t* cs, uint32_t lo_fix, uint32_t cx, uint32_t cy, bool live) {
    RowRanges R;
    for (int r = 0; r < 3; ++r) {
        R.lo[r] = 0; R.hi[r] = 0;
        if (live) (void)row_range(P, cs, cx, cy + (uint32_t)(r - 1), lo_fix, &R.lo[r], &R.hi[r]);
        if (R.hi[r] < R.lo[r]) R.hi[r] = R.lo[r];
    }
    return R;
}

int main() {
    unsigned long long cases = 0, bad = 0;
    uint32_t rng = 12345u;
    auto next = [&]() { rng = rng * 1664525u + 1013904223u; return rng >> 16; };
    for (uint32_t gu = 1; gu <= 6; ++gu)
        for (uint32_t gv = 1; gv <= 5; ++gv) {
            StepParams P{};
            P.grid_u = gu; P.grid_v = gv; P.ncell = gu * gv;
            for (int fillmode = 0; fillmode < 4; ++fillmode) {
                // the table has ncell + 1 entries; a guard word behind it catches a read past the end
                std::vector<uint32_t> cs(P.ncell + 1);
                uint32_t acc = 0;
                for (uint32_t c = 0; c <= P.ncell; ++c) {
                    if (fillmode == 0) cs[c] = acc += next() % 3;                       // a cell-start table: zeros in front, plateaus
                    else if (fillmode == 1) cs[c] = 0;                                  // empty
                    else if (fillmode == 2) cs[c] = c + 1;                              // no zero at all
                    else cs[c] = next() % 7;                                            // not monotone: hi < lo happens
                }
                const uint32_t coords_u[] = {0u, 1u, 2u, gu - 1u, gu, gu + 1u, 0xFFFFFFFFu, 0xFFFFFFFEu};
                const uint32_t coords_v[] = {0u, 1u, 2u, gv - 1u, gv, gv + 1u, 0xFFFFFFFFu, 0xFFFFFFFEu};
                for (uint32_t lo_fix = 0; lo_fix < 3; ++lo_fix)
                    for (uint32_t cx : coords_u)
                        for (uint32_t cy : coords_v)
                            for (int live = 0; live < 2; ++live) {
                                const RowRanges A = three_calls(P, cs.data(), lo_fix, cx, cy, live != 0);
                                const RowRanges B = lane_row_ranges(P, cs.data(), lo_fix, cx, cy, live != 0);
                                ++cases;
                                for (int r = 0; r < 3; ++r)
                                    if (A.lo[r] != B.lo[r] || A.hi[r] != B.hi[r]) {
                                        if (bad < 10)
                                            std::printf("grid %u x %u fill %d lo_fix %u cx %u cy %u live %d row %d: [%u, %u) vs [%u, %u)\n", gu, gv,
                                                        fillmode, lo_fix, cx, cy, live, r, A.lo[r], A.hi[r], B.lo[r], B.hi[r]);
                                        ++bad;
                                    }
                            }
            }
        }
    std::printf("cases %llu mismatches %llu\n", cases, bad);
    return bad ? 1 : 0;
}
