"""numpy restatement of "3D channel sampling" (include/fluidsim.h).  TEST INFRASTRUCTURE ONLY; written from the
header text, not from the kernel.

Every operation is one numpy f32 operation (one rounding, no contraction).  The queries are taken together, but each query's
sums grow in the statement's order: the 27 cells oz, oy, ox in -1..1, and within a cell the slots ascending — step j of a cell
adds, for every query whose cell still has a j-th slot and whose candidate is in radius, that candidate's term and nothing else
(a skipped candidate is not an added zero)."""
import ctypes
import ctypes.util

import numpy as np

from tests.track3d_ref import cell_xyz

f = np.float32
PI3 = f(3.14159265359)


_libm = None


def powf(x, y):
    """powf of the host libm, which the header's C6 names.  numpy's float32 power is another implementation: at h = 0.33 it is
    one ulp off, and so was every weight (tests/test_hard_states3d.py compares the two)."""
    global _libm
    if _libm is None:
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.powf.restype, _libm.powf.argtypes = ctypes.c_float, [ctypes.c_float, ctypes.c_float]
    return f(_libm.powf(float(f(x)), float(f(y))))


def poly6(h):
    """C6 = 315.0f / (64.0f * PI3 * powf(h, 9.0f))."""
    return f(315.0) / (f(64.0) * PI3 * powf(h, 9.0))


def sample_attr(settings, grid_dims, mass, p, attr, points, dtype=np.float32):
    """(weight[n], a[C, n]) at `points` over the records p (sorted by grid, as after a step) and the channels attr[C, len(p)].
    dtype=np.float64: the same sums in double (no statement; the yardstick of the tolerance comparison)."""
    T = dtype
    exact = T == np.float32
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    nq, n = pts.shape[0], p.shape[0]
    attr = np.asarray(attr, dtype=np.float32).reshape(-1, n)
    C = attr.shape[0]
    gw, gh, gd = (int(v) for v in grid_dims)
    grid = p["grid"].astype(np.int64)
    assert (np.diff(grid) >= 0).all(), "the records are not sorted by grid"
    h = f(settings.smoothing_radius)
    h2 = T(h * h)
    m = T(f(mass))
    c6 = T(poly6(h))
    c = cell_xyz(settings, pts).astype(np.int64)                 # u32 values
    weight = np.zeros(nq, dtype=T)
    a = np.zeros((C, nq), dtype=T)
    q_pos = pts.astype(T)
    pos, rho, at = p["predicted_position"].astype(T), p["density"].astype(T), attr.astype(T)
    for oz in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                X, Y, Z = (c[:, 0] + ox) & 0xFFFFFFFF, (c[:, 1] + oy) & 0xFFFFFFFF, (c[:, 2] + oz) & 0xFFFFFFFF
                valid = (X < gw) & (Y < gh) & (Z < gd)
                ident = (Z * gh + Y) * gw + X
                lo = np.searchsorted(grid, ident, side="left")
                hi = np.searchsorted(grid, ident, side="right")
                cnt = np.where(valid, hi - lo, 0)
                for j in range(int(cnt.max()) if nq else 0):
                    qs = np.flatnonzero(cnt > j)
                    k = lo[qs] + j
                    d = pos[k] - q_pos[qs]
                    r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
                    inr = ~(r2 > h2)
                    qs, k, r2 = qs[inr], k[inr], r2[inr]
                    e = h2 - r2
                    W = ((c6 * e) * e) * e
                    t = (m / rho[k]) * W
                    weight[qs] = weight[qs] + t
                    for ch in range(C):
                        a[ch, qs] = a[ch, qs] + t * at[ch, k]
                    assert not exact or (t.dtype == np.float32 and W.dtype == np.float32)
    return weight, a
