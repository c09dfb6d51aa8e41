"""CPU statement of the fluid diagnostics (include/fluidsim.h "fluid diagnostics" and "3D fluid diagnostics"),
written from the header's text and from nothing in the engine: numpy over the records a download returns and the channel arrays
the tracking downloads return.  Q is tests/body_loads2d_ref.py's, the one statement of it.  TEST INFRASTRUCTURE ONLY.

A result is a dict of Python ints: the integer words as they are, every float as its bit pattern (so that -0 and +0 differ and a
comparison is bit equality), vectors and per-channel fields as tuples.  `words_of` turns an fs_stats / fs3_stats record (the
ctypes structure) into the same dict."""
import numpy as np

from tests import body_loads2d_ref as B

f32, u32 = np.float32, np.uint32
SHIFT = B.SHIFT
MAX_CHANNELS = 4
POS_INF, NEG_INF = 0x7F800000, 0xFF800000           # where minima and maxima start, as bits
# crafted values the tests share
TIE_LO, TIE_MID, TIE_HI = f32(2.0 ** -21), f32(1.5 * 2.0 ** -20), f32(2.5 * 2.0 ** -20)     # x * 2^20 = 0.5, 1.5, 2.5
SMALL_Q = 1 << 16                 # up to here sums are sum(B.Q(x)) itself; above, its vectorised form (checked against it)


def bits(x):
    return np.ascontiguousarray(x, dtype=f32).view(u32)


def key(x):
    """the order-preserving u32 key of non-NaN floats: -inf < ... < -0 < +0 < ... < +inf"""
    b = bits(x).astype(np.uint64)
    return (b ^ np.where(b >> np.uint64(31) != 0, np.uint64(0xFFFFFFFF), np.uint64(0x80000000))).astype(u32)


def unkey_bits(k):
    """the bit pattern of the float a key stands for, a Python int"""
    k = int(k)
    return k ^ (0x80000000 if k & 0x80000000 else 0xFFFFFFFF)


def low_high(x):
    """(bits of the least, bits of the greatest) of finite values in the total order of bit patterns; the starting values when empty"""
    if x.size == 0:
        return POS_INF, NEG_INF
    k = key(x)
    return unkey_bits(k.min()), unkey_bits(k.max())


def q_sum(x):
    """sum of Q over values that are all in range, a Python int"""
    x = np.asarray(x, dtype=f32).reshape(-1)
    if x.size <= SMALL_Q:
        return sum(B.Q(x))
    assert B.in_range(x).all()
    q = np.rint(x.astype(np.float64) * 2 ** SHIFT).astype(np.int64)        # |q| < 2^34, fewer than 2^28 of them: no wrap
    assert q[:4096].tolist() == B.Q(x[:4096])
    return int(q.sum())


def stats(rec, attrs=(), tick=0):
    """The header's statement over the records `rec` (fields position, velocity [n, D] and density [n]) and the channel arrays
    `attrs` (each [n])."""
    n = rec.shape[0]
    p, v, rho = rec["position"], rec["velocity"], rec["density"]
    D = p.shape[1]
    assert len(attrs) <= MAX_CHANNELS and all(a.shape == (n,) for a in attrs)
    with np.errstate(all="ignore"):
        finite = np.isfinite(p).all(axis=1) & np.isfinite(v).all(axis=1) & np.isfinite(rho)
        p, v, rho = p[finite], v[finite], rho[finite]
        e = v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]                          # float32 products, float32 sum
        if D == 3:
            e = e + v[:, 2] * v[:, 2]
        e = e.astype(f32)
    keep = B.in_range(e) & B.in_range(rho)
    for a in range(D):
        keep &= B.in_range(p[:, a]) & B.in_range(v[:, a])
    out = {"count": n, "nonfinite": int((~finite).sum()), "dropped": int((~keep).sum()), "tick": int(tick), "channels": len(attrs)}
    out["momentum_q"] = tuple(q_sum(v[keep, a]) for a in range(D))
    out["energy_q"] = q_sum(e[keep])
    out["position_q"] = tuple(q_sum(p[keep, a]) for a in range(D))
    out["density_q"] = q_sum(rho[keep])
    out["speed2_max"] = low_high(e)[1]
    out["density_min"], out["density_max"] = low_high(rho)
    lh = [low_high(p[:, a]) for a in range(D)]
    out["pos_min"], out["pos_max"] = tuple(x[0] for x in lh), tuple(x[1] for x in lh)
    aq, ad, amin, amax = [0] * 4, [0] * 4, [POS_INF] * 4, [NEG_INF] * 4
    for c, a in enumerate(attrs):
        a = np.asarray(a, dtype=f32)
        fin = np.isfinite(a)
        ok = fin & B.in_range(a)
        aq[c], ad[c] = q_sum(a[ok]), int((~ok).sum())
        amin[c], amax[c] = low_high(a[fin])
    out["attr_q"], out["attr_dropped"], out["attr_min"], out["attr_max"] = tuple(aq), tuple(ad), tuple(amin), tuple(amax)
    return out


def _fbits(x):
    return int(np.array([x], dtype=f32).view(u32)[0])


def words_of(raw):
    """an fs_stats / fs3_stats ctypes record as the dict `stats` returns (plus nothing: `pad` must be 0)"""
    D = len(raw.momentum_q)
    assert int(raw.pad) == 0
    vec = lambda s: tuple(_fbits(getattr(s, a)) for a in "xyz"[:D])
    return {"count": int(raw.count), "nonfinite": int(raw.nonfinite), "dropped": int(raw.dropped), "tick": int(raw.tick),
            "channels": int(raw.channels), "momentum_q": tuple(int(x) for x in raw.momentum_q), "energy_q": int(raw.energy_q),
            "position_q": tuple(int(x) for x in raw.position_q), "density_q": int(raw.density_q),
            "speed2_max": _fbits(raw.speed2_max), "density_min": _fbits(raw.density_min), "density_max": _fbits(raw.density_max),
            "pos_min": vec(raw.pos_min), "pos_max": vec(raw.pos_max), "attr_q": tuple(int(x) for x in raw.attr_q),
            "attr_dropped": tuple(int(x) for x in raw.attr_dropped), "attr_min": tuple(_fbits(x) for x in raw.attr_min),
            "attr_max": tuple(_fbits(x) for x in raw.attr_max)}


def assert_same(got, want, ctx=""):
    """every word, integer and bit equality; the message names the fields that differ"""
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad and set(got) == set(want), f"{ctx}: (got, want) {bad}"


def kept(w):
    """count - nonfinite - dropped: the records in every sum"""
    return w["count"] - w["nonfinite"] - w["dropped"]


# ---- the crafted records, with their words written out by hand ------------------------------------------------------------------
def _records(dtype, rows):
    """records of `dtype` from rows (position..., velocity..., density); every other field zero"""
    D = np.zeros(1, dtype=dtype)["position"].shape[1]
    rec = np.zeros(len(rows), dtype=dtype)
    for i, r in enumerate(rows):
        rec["position"][i] = f32(r[:D])
        rec["velocity"][i] = f32(r[D:2 * D])
        rec["density"][i] = f32(r[2 * D])
    rec["predicted_position"] = rec["position"]
    return rec


Q1 = 1 << SHIFT                   # Q(1.0)
_NAN = float("nan")


def crafted(dtype):
    """(records, channel arrays, the words by hand) of the crafted set: a Q tie on each side of zero (record 0), a position of
    exactly 2^14 (record 1: dropped, yet in the extremes), v = 1e20 (record 2: e = +inf, dropped, speed2_max = +inf), a NaN
    density (record 3: nonfinite, in nothing — its position would be the minimum), an ordinary record (4)."""
    D = np.zeros(1, dtype=dtype)["position"].shape[1]
    if D == 2:
        rows = [(-TIE_LO, -TIE_MID, TIE_LO, TIE_MID, TIE_HI), (16384.0, 1.0, 1.0, 2.0, 3.0), (2.0, -3.0, 1e20, 0.0, 1.0),
                (-99999.0, 7.0, 1.0, 1.0, _NAN), (1.5, -2.25, -3.0, 4.0, 1000.5)]
    else:
        rows = [(-TIE_LO, -TIE_MID, TIE_LO, TIE_LO, TIE_MID, -TIE_HI, TIE_HI), (16384.0, 1.0, 0.5, 1.0, 2.0, 0.0, 3.0),
                (2.0, -3.0, 0.0, 1e20, 0.0, 0.0, 1.0), (-99999.0, 7.0, -99999.0, 1.0, 1.0, 1.0, _NAN),
                (1.5, -2.25, 0.5, -3.0, 4.0, 12.0, 1000.5)]
    attrs = [f32([TIE_LO, 16384.0, _NAN, -TIE_MID, 3.0]), f32([-0.0, 0.0, np.inf, -np.inf, 1e30])]
    # record 0: Q(-0.5 ulp) = 0, Q(-1.5) = -2, Q(0.5) = 0, Q(1.5) = 2, Q(2.5) = 2 (3D: Q of vz = -2.5 is -2), e rounds to 0
    want = {"count": 5, "nonfinite": 1, "dropped": 2, "tick": 0, "channels": 2,
            "density_q": 2 + 1000 * Q1 + Q1 // 2,
            "speed2_max": POS_INF, "density_min": _fbits(TIE_HI), "density_max": _fbits(1000.5),
            "attr_q": (0 + 3 * Q1 - 2, 0, 0, 0), "attr_dropped": (2, 3, 0, 0),
            "attr_min": (_fbits(-TIE_MID), 0x80000000, POS_INF, POS_INF), "attr_max": (_fbits(16384.0), _fbits(1e30), NEG_INF, NEG_INF)}
    if D == 2:
        want.update({"momentum_q": (0 - 3 * Q1, 2 + 4 * Q1), "energy_q": 0 + 25 * Q1, "position_q": (0 + Q1 + Q1 // 2, -2 - 2 * Q1 - Q1 // 4),
                     "pos_min": (_fbits(-TIE_LO), _fbits(-3.0)), "pos_max": (_fbits(16384.0), _fbits(1.0))})
    else:
        want.update({"momentum_q": (0 - 3 * Q1, 2 + 4 * Q1, -2 + 12 * Q1), "energy_q": 0 + 169 * Q1,
                     "position_q": (0 + Q1 + Q1 // 2, -2 - 2 * Q1 - Q1 // 4, 0 + Q1 // 2),
                     "pos_min": (_fbits(-TIE_LO), _fbits(-3.0), 0), "pos_max": (_fbits(16384.0), _fbits(1.0), _fbits(0.5))})
    return _records(dtype, rows), attrs, want


def crafted_zeros(dtype):
    """(records, no channels, the words by hand): two records whose positions are -0 and +0 only: pos_min is -0 and pos_max +0 by bits"""
    D = np.zeros(1, dtype=dtype)["position"].shape[1]
    if D == 2:
        rows = [(-0.0, 0.0, 0.25, -0.5, 2.0), (0.0, -0.0, -0.25, 0.5, 2.0)]
    else:
        rows = [(-0.0, 0.0, -0.0, 0.25, -0.5, 0.0, 2.0), (0.0, -0.0, 0.0, -0.25, 0.5, 0.0, 2.0)]
    want = {"count": 2, "nonfinite": 0, "dropped": 0, "tick": 0, "channels": 0, "momentum_q": (0,) * D, "energy_q": 2 * (Q1 // 16 + Q1 // 4),
            "position_q": (0,) * D, "density_q": 4 * Q1, "speed2_max": _fbits(0.3125), "density_min": _fbits(2.0), "density_max": _fbits(2.0),
            "pos_min": (0x80000000,) * D, "pos_max": (0,) * D, "attr_q": (0,) * 4, "attr_dropped": (0,) * 4,
            "attr_min": (POS_INF,) * 4, "attr_max": (NEG_INF,) * 4}
    return _records(dtype, rows), [], want


def crafted_empty(dtype):
    """(records, no channels, the words by hand) of the empty-sums case: every record is non-finite, so nothing contributes and the
    extremes stay where they start"""
    D = np.zeros(1, dtype=dtype)["position"].shape[1]
    rows = [(1.0,) * D + (2.0,) * D + (_NAN,), (np.inf,) + (0.0,) * (2 * D - 1) + (1.0,), (0.0,) * D + (-np.inf,) + (0.0,) * (D - 1) + (1.0,)]
    want = {"count": 3, "nonfinite": 3, "dropped": 0, "tick": 0, "channels": 0, "momentum_q": (0,) * D, "energy_q": 0, "position_q": (0,) * D,
            "density_q": 0, "speed2_max": NEG_INF, "density_min": POS_INF, "density_max": NEG_INF, "pos_min": (POS_INF,) * D,
            "pos_max": (NEG_INF,) * D, "attr_q": (0,) * 4, "attr_dropped": (0,) * 4, "attr_min": (POS_INF,) * 4, "attr_max": (NEG_INF,) * 4}
    return _records(dtype, rows), [], want
