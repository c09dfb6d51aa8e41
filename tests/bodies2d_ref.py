"""CPU statement of the 2D moving bodies (include/fluidsim.h "2D moving bodies"), written from the header's text
and from nothing in the kernel: the operator B of one body in numpy float32, one f32 operation per line, the scene of three
moving bodies the tests share, and the oracle run that goes with it (the unchanged 2D oracle, its texture push-out included, then
B_0 .. B_7 on its records after every step).  TEST INFRASTRUCTURE ONLY.

Arrays follow the Python API: a field is float32 [H, W, 2], a mask uint8 [H, W]; pixel (i, j) is [j, i]."""
import numpy as np

from tests import collide3d_ref as CR

f32 = np.float32
IDENTITY = (1.0, 0.0, 0.0, 1.0)


class Body:
    """one body as the operator takes it: field [H, W, 2], the box extent, and the motion, every float a float32"""

    def __init__(self, field, extent, centre=(0.0, 0.0), rot=IDENTITY, velocity=(0.0, 0.0), angular_velocity=0.0):
        self.field = np.asarray(field, dtype=f32)
        self.extent = np.array([f32(e) for e in extent], dtype=f32)
        self.set_motion(centre, rot, velocity, angular_velocity)

    def set_motion(self, centre, rot=IDENTITY, velocity=(0.0, 0.0), angular_velocity=0.0):
        self.centre = np.array([f32(x) for x in centre], dtype=f32)
        self.rot = np.asarray(rot, dtype=f32).reshape(4).copy()
        self.velocity = np.array([f32(x) for x in velocity], dtype=f32)
        self.angular_velocity = f32(angular_velocity)
        return self

    def motion(self):
        """the arguments of FluidSimulation.set_body_motion after the slot"""
        return self.centre, self.rot, self.velocity, self.angular_velocity


def apply_body_record(records, body, size, damping):
    """B(records) with what the loads need of every hit (tests/body_loads2d_ref.py): (new records, rec) — rec["hit"]: bool per
    particle; per HIT, in particle order: rec["v0"], rec["v1"], rec["s"] float32 [hits, 2] and rec["clamped"] bool [hits].
    `size`: the settings' box, `damping`: the tick's damping_factor."""
    field = body.field
    H, W = field.shape[:2]
    out = records.copy()
    p = out["position"].astype(f32)
    v = out["velocity"].astype(f32)
    b = np.array([f32(s) for s in size], dtype=f32) * f32(0.5)
    damping = f32(damping)
    c, r, u, w, ext = body.centre, body.rot, body.velocity, body.angular_velocity, body.extent
    r00, r01, r10, r11 = (f32(x) for x in r)
    with np.errstate(all="ignore"):
        hb = ext * f32(0.5)
        dx = p[:, 0] - c[0]
        dy = p[:, 1] - c[1]
        t0 = r00 * dx
        t1 = r10 * dy
        qx = t0 + t1
        t0 = r01 * dx
        t1 = r11 * dy
        qy = t0 + t1
        inside = (np.abs(qx) <= hb[0]) & (np.abs(qy) <= hb[1])
        idx = []
        for a, (q, wa) in enumerate(((qx, W), (qy, H))):
            x = q + hb[a]
            x = x / ext[a]
            x = x * f32(wa)
            idx.append(np.minimum(CR.u32_sat(x), np.uint64(wa - 1)).astype(np.int64))
        g = field[idx[1], idx[0]]
        nz = (g[:, 0] != 0) | (g[:, 1] != 0)
        t0 = g[:, 0] * g[:, 0]
        t1 = g[:, 1] * g[:, 1]
        ln = np.sqrt(t0 + t1)
        hit = inside & nz & (ln > f32(0))
        g, ln, ph, vh = g[hit], ln[hit], p[hit], v[hit]
        v0 = vh.copy()                                  # the velocity on entry to this operator
        t0 = r00 * g[:, 0]
        t1 = r01 * g[:, 1]
        fx = t0 + t1
        t0 = r10 * g[:, 0]
        t1 = r11 * g[:, 1]
        fy = t0 + t1
        nx = fx / ln
        ny = fy / ln
        px = ph[:, 0] + fx
        py = ph[:, 1] + fy
        sx = px - c[0]
        sy = py - c[1]
        t0 = w * sy
        usx = u[0] - t0
        t0 = w * sx
        usy = u[1] + t0
        rx = vh[:, 0] - usx
        ry = vh[:, 1] - usy
        t0 = rx * nx
        t1 = ry * ny
        rn = t0 + t1
        k = (f32(1.0) - damping) * rn
        t0 = k * nx
        t0 = rx - t0
        vx = usx + t0
        t0 = k * ny
        t0 = ry - t0
        vy = usy + t0
        ph = np.stack([px, py], axis=1).astype(f32).reshape(-1, 2)
        vh = np.stack([vx, vy], axis=1).astype(f32).reshape(-1, 2)
        v1 = vh.copy()                                  # before the wall re-clamp
        s = np.stack([sx, sy], axis=1).astype(f32).reshape(-1, 2)
        clamped = np.zeros(ph.shape[0], dtype=bool)
        for a in range(2):
            over = np.abs(ph[:, a]) > b[a]
            ph[over, a] = b[a] * np.sign(ph[over, a])
            vh[over, a] = vh[over, a] * (f32(-1.0) * damping)
            clamped |= over
    p[hit] = ph
    v[hit] = vh
    out["position"] = p
    out["velocity"] = v
    return out, {"hit": hit, "v0": v0, "v1": v1, "s": s, "clamped": clamped}


def apply_body(records, body, size, damping):
    """B(records): (new records, particles hit, particles re-clamped after their push)"""
    out, rec = apply_body_record(records, body, size, damping)
    return out, int(rec["hit"].sum()), int(rec["clamped"].sum())


def apply_bodies(records, bodies, size, damping):
    """B_last(... B_first(records)) in the order given: (new records, hits per body, re-clamps per body)"""
    hits, clamps = [], []
    for body in bodies:
        records, h, c = apply_body(records, body, size, damping)
        hits.append(h)
        clamps.append(c)
    return records, hits, clamps


def producer_field(mask, extent):
    """fs_body_create_from_mask's field of a uint8 [H, W] mask over the box `extent`: the 3D producer on the w x h x 1 mask, z dropped"""
    return np.ascontiguousarray(CR.producer_field(np.asarray(mask, dtype=np.uint8)[None], (extent[0], extent[1], 1.0))[0, :, :, :2])


def random_field(shape_wh, seed, fill=0.5, mag=0.15):
    """[H, W, 2] with about `fill` of the pixels non-zero, components up to `mag`"""
    w, h = shape_wh
    rng = np.random.default_rng(seed)
    f = rng.uniform(-mag, mag, size=(h, w, 2)).astype(f32)
    f[rng.random((h, w)) >= fill] = 0
    return f


# ---- the shared scene: a paddle, a stirrer and a tilted slab in dam_break_2d ------------------------------------------------
def solid_except(shape_hw, axis, free):
    """a mask that is solid (255) except the slices `free` along `axis` (0: y, 1: x)"""
    m = np.full(shape_hw, 255, dtype=np.uint8)
    sl = [slice(None)] * 2
    for f in free:
        sl[axis] = f
        m[tuple(sl)] = 0
    return m


class Scene:
    """The three bodies of dam_break_2d(side^2) and their motion per step.  Slot order: paddle, stirrer, slab.  The block of
    fluid lies against the -x wall on the floor (+y: gravity points there)."""

    def __init__(self, fs, side):
        st, off, tick = fs.dam_break_2d(side ** 2)
        self.fs, self.st, self.off, self.tick = fs, st, off, tick
        self.size = (st.size.x, st.size.y)
        sx, sy = (float(s) for s in self.size)
        L = side * 0.1
        self.dt = f32(tick.delta)
        # the paddle pushes along x out of its two free edge columns and runs from inside the block to the -x wall (from step 14
        # on its left half pushes through that wall), the stirrer pushes across its thickness, the slab out of its one free edge
        # row: with the slab's centre on the floor and that row below it, its push goes through the floor
        self.masks = [solid_except((4, 8), 1, (0, -1)), solid_except((5, 10), 0, (0, -1)), solid_except((6, 4), 0, (-1,))]
        self.extents = [(1.2, sy), (1.2, 0.3), (0.8, 0.6)]
        self.paddle_u = np.array([-3.0, 0.0], dtype=f32)
        self.paddle_c0 = np.array([-sx / 2 + 0.9, 0.0], dtype=f32)
        self.stirrer_c = (-sx / 2 + 0.5 * L, sy / 2 - 2.0)
        self.slab_c = (-sx / 2 + 0.5 * L, sy / 2)
        self.slab_rot = fs.rigid_motion2d(self.slab_c, (0, 0), 0.3, 1.0)[1]
        self.fields = [producer_field(m, e) for m, e in zip(self.masks, self.extents)]

    def bodies(self):
        """fresh Body objects, motion not yet set"""
        return [Body(f, e) for f, e in zip(self.fields, self.extents)]

    def set_motions(self, bodies, s):
        """the motion of step s = 1, 2, ... into `bodies`: the paddle's centre is advanced by u * dt in f32 once per step (step 1
        starts from the start position), the stirrer is turned by 4 * s * dt, the slab rests"""
        c = self.paddle_c0.copy()
        for _ in range(s - 1):
            c = c + self.paddle_u * self.dt
        bodies[0].set_motion(c, IDENTITY, self.paddle_u)
        sc, srot = self.fs.rigid_motion2d(self.stirrer_c, (0, 0), 4.0, float(s) * float(self.dt))
        bodies[1].set_motion(sc, srot, (0, 0), 4.0)
        bodies[2].set_motion(self.slab_c, self.slab_rot)
        return bodies

    def texture(self):
        """a non-zero force texture (pixel units, [th, tw, 2]): a band of the block, through the stirrer's and the slab's place,
        pushed two pixels right and one up by the reference step itself, before any body"""
        tw, th = int(self.st.texture_size.x), int(self.st.texture_size.y)
        t = np.zeros((th, tw, 2), dtype=f32)
        t[:, tw // 5: tw // 4] = (2.0, -1.0)
        return t


_RUNS = {}


def oracle_run(fs, orc, side, sort="bitonic", texture=False, steps=40, keep=(1, 8, 40)):
    """The scene on the CPU: the unchanged 2D oracle (stable_sort=True for the counting-sort handle), then the three operators,
    applied to its records after every step.  {"snap": {step: records}, "hits": per-body hits per step [steps, 3], "reclamped":
    likewise, "scene": Scene, "texture": field or None}; computed once, never changed."""
    key = (side, sort, texture, steps, tuple(keep))
    if key not in _RUNS:
        sc = Scene(fs, side)
        bodies = sc.bodies()
        ref = orc.OracleSim(sc.st, initial_offset=sc.off)
        tex = sc.texture() if texture else None
        if texture:
            ref.texture_view()[:] = tex
        snap, hits, clamps = {}, [], []
        for s in range(1, steps + 1):
            ref.step(sc.tick, stable_sort=sort == "counting")
            rec, h, c = apply_bodies(ref.particles(), sc.set_motions(bodies, s), sc.size, sc.tick.damping_factor)
            ref.set_particles(rec)
            hits.append(h)
            clamps.append(c)
            if s in keep:
                snap[s] = rec
        ref.close()
        for r in snap.values():
            r.setflags(write=False)
        _RUNS[key] = {"snap": snap, "hits": np.array(hits), "reclamped": np.array(clamps), "scene": sc, "texture": tex}
    return _RUNS[key]
