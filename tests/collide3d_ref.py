"""CPU statement of the 3D colliders (include/fluidsim.h "3D colliders"), written from the header's text and from
nothing in the kernels: the operator C in numpy float32, the three producer passes in integer numpy, a brute-force nearest-free
distance, and the two hand-built scenes the tests share.  TEST INFRASTRUCTURE ONLY.

Arrays follow the Python API: a field is float32 [D, H, W, 3], a mask uint8 [D, H, W]; voxel (i, j, k) is [k, j, i]."""
import numpy as np

f32 = np.float32
NONE = -1


# ---- the operator C ---------------------------------------------------------------------------------------------------
def u32_sat(x):
    """oracle/sph_oracle3d.cpp u32sat on a float32 array: NaN and non-positive -> 0, >= 2^32 -> 2^32 - 1, else truncation."""
    x = np.asarray(x, dtype=f32)
    out = np.zeros(x.shape, dtype=np.uint64)
    with np.errstate(invalid="ignore"):
        pos = x > f32(0)
        big = x >= f32(4294967296.0)
    mid = pos & ~big
    out[mid] = x[mid].astype(np.uint64)
    out[big] = 0xFFFFFFFF
    return out


def apply_collider(records, field, size, damping):
    """C(records): (new records, particles pushed, particles re-clamped after a push).  `size`: the settings' box (3 floats),
    `damping`: the tick's damping_factor.  Every operation is one float32 operation, in the header's order."""
    field = np.asarray(field, dtype=f32)
    D, H, W = field.shape[:3]
    out = records.copy()
    p = out["position"].astype(f32)             # copies: [n, 3]
    v = out["velocity"].astype(f32)
    size = np.array([f32(s) for s in size], dtype=f32)
    b = size * f32(0.5)
    damping = f32(damping)
    with np.errstate(all="ignore"):
        idx = []
        for a, wa in enumerate((W, H, D)):
            x = ((p[:, a] + b[a]) / size[a]) * f32(wa)
            idx.append(np.minimum(u32_sat(x), np.uint64(wa - 1)).astype(np.int64))
        f = field[idx[2], idx[1], idx[0]]                                     # [n, 3]
        nz = (f[:, 0] != 0) | (f[:, 1] != 0) | (f[:, 2] != 0)
        ln = np.sqrt((f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2])
        hit = nz & (ln > f32(0))
        fh, lh, ph, vh = f[hit], ln[hit], p[hit], v[hit]
        n = fh / lh[:, None]
        ph = ph + fh
        vn = (vh[:, 0] * n[:, 0] + vh[:, 1] * n[:, 1]) + vh[:, 2] * n[:, 2]
        k = (f32(1.0) - damping) * vn
        vh = vh - k[:, None] * n
        clamped = np.zeros(ph.shape[0], dtype=bool)
        for a in range(3):
            over = np.abs(ph[:, a]) > b[a]
            ph[over, a] = b[a] * np.sign(ph[over, a])
            vh[over, a] = vh[over, a] * (f32(-1.0) * damping)
            clamped |= over
    p[hit] = ph
    v[hit] = vh
    out["position"] = p
    out["velocity"] = v
    return out, int(hit.sum()), int(clamped.sum())


def random_field(shape_whd, seed, fill=0.5, mag=0.15):
    """[D, H, W, 3] with about `fill` of the voxels non-zero, components up to `mag`"""
    w, h, d = shape_whd
    rng = np.random.default_rng(seed)
    f = rng.uniform(-mag, mag, size=(d, h, w, 3)).astype(f32)
    f[rng.random((d, h, w)) >= fill] = 0
    return f


# ---- the producer -----------------------------------------------------------------------------------------------------
def _argmin_first(cost, axis):
    """index of the first minimum along `axis` and the minimum: ties go to the smaller coordinate"""
    j = np.argmin(cost, axis=axis)
    return j, np.take_along_axis(cost, np.expand_dims(j, axis), axis).squeeze(axis)


def producer_passes(mask):
    """The X, Y and Z passes on a uint8 [D, H, W] mask: (c, d2) with c int64 [D, H, W, 3] = the (x, y, z) index of the voxel each
    voxel is sent to (NONE everywhere if the mask has no free voxel) and d2 its squared index distance."""
    mask = np.asarray(mask, dtype=np.uint8)
    D, H, W = mask.shape
    BIG = np.int64(1) << 40
    free = ~(mask > 128)
    ii, jj, kk = np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64), np.arange(D, dtype=np.int64)
    # X: cost[k, j, i, i'] = |i - i'| over free i'
    cost = np.where(free[:, :, None, :], np.abs(ii[:, None] - ii[None, :])[None, None], BIG)
    a, m = _argmin_first(cost, 3)
    a = np.where(m < BIG, a, NONE)                                            # [D, H, W]
    # Y: cost[k, j, j', i] = (a(i, j', k) - i)^2 + (j' - j)^2 over defined a
    dx2 = (a - ii[None, None, :]) ** 2                                        # [D, H(j'), W]
    cost = np.where((a != NONE)[:, None, :, :], dx2[:, None, :, :] + ((jj[None, :] - jj[:, None]) ** 2)[None, :, :, None], BIG)
    jb, m = _argmin_first(cost, 2)                                            # [D, H, W]
    bx = np.where(m < BIG, np.take_along_axis(a, jb, 1), NONE)
    by = np.where(m < BIG, jb, NONE)
    # Z: cost[k, k', j, i] = (b.x - i)^2 + (b.y - j)^2 + (k' - k)^2 over defined b
    dxy2 = (bx - ii[None, None, :]) ** 2 + (by - jj[None, :, None]) ** 2      # [D(k'), H, W]
    cost = np.where((bx != NONE)[None], dxy2[None] + ((kk[None, :] - kk[:, None]) ** 2)[:, :, None, None], BIG)
    kb, m = _argmin_first(cost, 1)                                            # [D, H, W]
    ok = m < BIG
    c = np.stack([np.where(ok, _gather0(bx, kb), NONE), np.where(ok, _gather0(by, kb), NONE), np.where(ok, kb, NONE)], axis=-1)
    return c, np.where(ok, m, NONE)


def _gather0(arr, k):
    """arr[k[z, y, x], y, x]"""
    D, H, W = arr.shape
    return arr[k, np.arange(H)[None, :, None], np.arange(W)[None, None, :]]


def producer_field(mask, size):
    """The push field of a mask over a box of `size`: float32 [D, H, W, 3]; a free voxel's vector is exactly +0."""
    c, _ = producer_passes(mask)
    D, H, W = np.asarray(mask).shape
    out = np.zeros((D, H, W, 3), dtype=f32)
    if (c == NONE).any():
        return out
    own = np.stack(np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")[::-1], axis=-1)   # (i, j, k) per voxel
    for a, wa in enumerate((W, H, D)):
        s = f32(size[a]) / f32(wa)
        out[..., a] = (c[..., a] - own[..., a]).astype(np.int32).astype(f32) * s
    return out


def brute_nearest_d2(mask):
    """the true minimum squared index distance from every voxel to a free voxel: int64 [D, H, W]"""
    mask = np.asarray(mask, dtype=np.uint8)
    D, H, W = mask.shape
    kji = np.stack(np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)
    fr = kji[~(mask.reshape(-1) > 128)]
    d2 = ((kji[:, None, :] - fr[None, :, :]) ** 2).sum(-1)
    return d2.min(axis=1).reshape(D, H, W)


# ---- the hand-built scenes of the oracle comparison ---------------------------------------------------------------------
def voxel_centres(size, shape):
    """world coordinates of the voxel centres of a [D, H, W] field: three float64 arrays [W], [H], [D]"""
    D, H, W = shape
    return [(np.arange(n) + 0.5) / n * float(size[a]) - float(size[a]) / 2 for a, n in enumerate((W, H, D))]


def scene_box_on_floor(size, shape=None):
    """(a) a box standing on the floor (+y: gravity of dam_break_3d points there) in the dam's path, right of the initial block,
    across the whole depth.  Its voxels push out through the box's nearer x-face, by the distance to that face plus a tenth of a
    voxel: hand-built, not the producer's field."""
    sx, sy, sz = (float(s) for s in size)
    if shape is None:
        shape = (max(1, int(round(sz / 0.1))), max(1, int(round(sy / 0.1))), max(1, int(round(sx / 0.1))))
    X, Y, _ = voxel_centres(size, shape)
    x0, x1 = 0.05 * sx, 0.05 * sx + 0.4          # the block ends just left of x = 0
    y0 = sy / 2 - 0.6
    f = np.zeros(tuple(shape) + (3,), dtype=f32)
    vox = sx / shape[2]
    inx = (X >= x0) & (X <= x1)
    iny = Y >= y0
    left = X - x0 <= x1 - X
    push = np.where(left, -(X - x0) - 0.1 * vox, (x1 - X) + 0.1 * vox)
    f[:, :, :, 0] = np.where(inx[None, None, :] & iny[None, :, None], push[None, None, :], 0.0).astype(f32)
    return f


def scene_layer_through_wall(size, shape=(3, 5, 16)):
    """(b) a solid layer along the -x wall, overlapping the initial block, whose vectors point through that wall (and a little
    up): every particle it pushes leaves the box and is clamped again."""
    sx = float(size[0])
    X, _, _ = voxel_centres(size, shape)
    f = np.zeros(tuple(shape) + (3,), dtype=f32)
    layer = X < -sx / 2 + 0.45
    f[:, :, layer, 0] = f32(-0.75)
    f[:, :, layer, 1] = f32(-0.05)
    return f


_ORACLE_RUNS = {}


def oracle_run(fs, orc, side, scene, steps=40, keep=(1, 8, 40)):
    """dam_break_3d(side^3) under scene 'a' / 'b' on the CPU: the unchanged 3D oracle with C applied to its records after every
    step.  {"snap": {step: records}, "pushed": total, "reclamped": total, "field": field}; computed once, never changed."""
    key = (side, scene, steps, tuple(keep))
    if key not in _ORACLE_RUNS:
        st, off, tick = fs.dam_break_3d(side ** 3)
        size = (st.size.x, st.size.y, st.size.z)
        field = scene_box_on_floor(size) if scene == "a" else scene_layer_through_wall(size)
        ref = orc.OracleSim3D(st, initial_offset=off)
        snap, pushed, reclamped = {}, 0, 0
        for s in range(1, steps + 1):
            ref.step(tick)
            rec, np_, nc = apply_collider(ref.particles(), field, size, tick.damping_factor)
            ref.set_particles(rec)
            pushed += np_
            reclamped += nc
            if s in keep:
                snap[s] = rec
        ref.close()
        for r in snap.values():
            r.setflags(write=False)
        field.setflags(write=False)
        _ORACLE_RUNS[key] = {"snap": snap, "pushed": pushed, "reclamped": reclamped, "field": field}
    return _ORACLE_RUNS[key]
