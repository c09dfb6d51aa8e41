// force_identities_checker.cpp — the two f32 identities the strict force walk's shared-reciprocal terms rest on
// (csrc/fs_force_pair.h force_terms_shared), enumerated on the CPU.  TEST INFRASTRUCTURE ONLY; stand-alone (no oracle source),
// compiled with -ffp-contract=off by tests/checker_lib.py and driven by tests/test_force_identities.py.
//
//   fic_rim(lo, hi)            every f32 h with bits in [lo, hi]: is RN(sqrt(RN(h * h))) <= h ?  -> the number of h for which it is
//                              not.  With sqrt monotone this is "a pair the scan admitted, r2 <= RN(h * h), has dst <= h".
//   fic_half_quotient(h, n)    for every dst of the four binades below h (every mantissa, dst >= 2^-20), with y = RN(1 / dst):
//                              div_by_rcp(h, 2 dst, y / 2) == div_by_rcp(h / 2, dst, y) bit for bit?  -> the number of dst for which
//                              it is not; *n receives the number of pairs compared.
#include <cmath>
#include <cstdint>
#include <cstring>

namespace {

float f_of(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
uint32_t b_of(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

// csrc/fs_device.h div_by_rcp: q0 = RN(a y), r = fma(-q0, b, a), fma(r, y, q0)
float div_by_rcp(float a, float b, float y) {
    const float q0 = a * y;
    const float r = std::fmaf(-q0, b, a);
    return std::fmaf(r, y, q0);
}

}  // namespace

extern "C" {

uint64_t fic_rim(uint32_t lo_bits, uint32_t hi_bits) {
    uint64_t bad = 0;
#pragma omp parallel for reduction(+ : bad) schedule(static)
    for (int64_t b = lo_bits; b <= (int64_t)hi_bits; ++b) {
        const float h = f_of((uint32_t)b);
        const float hh = h * h;                 // sqr_radius as the host forms it
        const float d = std::sqrt(hh);          // IEEE: correctly rounded
        bad += !(d <= h);
    }
    return bad;
}

uint64_t fic_half_quotient(float h, uint64_t* compared) {
    int e;
    const float m = std::frexp(h, &e);          // h = m * 2^e, m in [0.5, 1)
    const int up = m == 0.5f ? e - 1 : e;       // ceil(log2 h)
    const uint32_t top = b_of(h);               // dst <= h
    // the four binades that hold values below h (h's own, when h is no power of two, and the ones under it), from 2^-20 up: the
    // shared-reciprocal path takes no smaller dst
    const float low = std::ldexp(1.0f, up - 4);
    const uint32_t bot = b_of(low < 0x1p-20f ? 0x1p-20f : low);
    uint64_t bad = 0, n = 0;
#pragma omp parallel for reduction(+ : bad, n) schedule(static)
    for (int64_t b = bot; b <= (int64_t)top; ++b) {
        const float dst = f_of((uint32_t)b);
        const float y = 1.0f / dst;
        const float was = div_by_rcp(h, 2.0f * dst, 0.5f * y);
        const float now = div_by_rcp(0.5f * h, dst, y);
        bad += b_of(was) != b_of(now);
        ++n;
    }
    *compared = n;
    return bad;
}

}  // extern "C"
