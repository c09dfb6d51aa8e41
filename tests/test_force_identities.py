"""The two f32 identities behind the strict force walk's shared-reciprocal terms (csrc/fs_force_pair.h force_terms_shared),
enumerated on the CPU by tests/force_identities_checker.cpp (compiled with the oracle's flags: no contraction).  No GPU.

  rim            RN(sqrt(RN(h * h))) <= h for EVERY f32 h of [2^-19, 2^19], the range the host enables the path for: a pair the scan
                 admitted by !(r2 > sqr_radius) has dst <= h, so force_terms_shared needs no `dst <= h` test of its own;
  half quotient  div_by_rcp(h, 2 dst, RN(1/dst) / 2) == div_by_rcp(h / 2, dst, RN(1/dst)) bit for bit, for
                 h in {0.35, 1, pi, 2^-19, 2^19} and every dst of the four binades below h: h / (2 dst) in three instructions."""
import ctypes as C
import functools

import numpy as np

from tests import checker_lib as CL

SOURCES = [CL.here("force_identities_checker.cpp")]
H_LO, H_HI = np.float32(2.0 ** -19), np.float32(2.0 ** 19)
HALF_QUOTIENT_H = (0.35, 1.0, float(np.float32(np.pi)), 2.0 ** -19, 2.0 ** 19)
HALF_QUOTIENT_PAIRS = 133_972_755


@functools.lru_cache(maxsize=None)
def lib():
    L = C.CDLL(CL.build("force_identities_checker", SOURCES))
    L.fic_rim.restype, L.fic_rim.argtypes = C.c_uint64, [C.c_uint32, C.c_uint32]
    L.fic_half_quotient.restype, L.fic_half_quotient.argtypes = C.c_uint64, [C.c_float, C.POINTER(C.c_uint64)]
    return L


def bits(x):
    return int(np.float32(x).view(np.uint32))


def test_the_checker_is_compiled_without_contraction():
    assert any(f.endswith("contract=off") for f in CL.FLAGS)      # the flag itself is spelled in oracle/oracle.py only


def test_sqrt_of_the_squared_radius_never_exceeds_the_radius():
    lo, hi = bits(H_LO), bits(H_HI)
    assert hi - lo + 1 == 318_767_105                       # every f32 of [2^-19, 2^19]
    assert lib().fic_rim(lo, hi) == 0


def test_the_rim_check_can_fail():
    """the same loop over h for which h * h overflows: sqrt(inf) <= h is false"""
    lo = bits(2.0 ** 100)
    assert lib().fic_rim(lo, lo + 99) == 100


def test_half_quotient_equals_the_quotient_by_twice_the_distance():
    total = 0
    for h in HALF_QUOTIENT_H:
        n = C.c_uint64(0)
        assert lib().fic_half_quotient(C.c_float(h), C.byref(n)) == 0, h
        total += n.value
    assert total == HALF_QUOTIENT_PAIRS
