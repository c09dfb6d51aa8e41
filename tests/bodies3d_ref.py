"""CPU statement of the 3D moving bodies (include/fluidsim.h "3D moving bodies"), written from the header's text
and from nothing in the kernel: the operator B of one body in numpy float32, one f32 operation per line, the scene of three
moving bodies the tests share, and the oracle run that goes with it (the unchanged 3D oracle, then C if a static collider is set,
then B_0 .. B_7 on its records after every step).  TEST INFRASTRUCTURE ONLY.

Arrays follow the Python API: a field is float32 [D, H, W, 3], a mask uint8 [D, H, W]; voxel (i, j, k) is [k, j, i]."""
import numpy as np

from tests import collide3d_ref as CR

f32 = np.float32
IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


class Body:
    """one body as the operator takes it: field [D, H, W, 3], the box extent, and the motion, every float a float32"""

    def __init__(self, field, extent, centre=(0.0, 0.0, 0.0), rot=IDENTITY, velocity=(0.0, 0.0, 0.0), angular_velocity=(0.0, 0.0, 0.0)):
        self.field = np.asarray(field, dtype=f32)
        self.extent = np.array([f32(e) for e in extent], dtype=f32)
        self.set_motion(centre, rot, velocity, angular_velocity)

    def set_motion(self, centre, rot=IDENTITY, velocity=(0.0, 0.0, 0.0), angular_velocity=(0.0, 0.0, 0.0)):
        self.centre = np.array([f32(x) for x in centre], dtype=f32)
        self.rot = np.asarray(rot, dtype=f32).reshape(9).copy()
        self.velocity = np.array([f32(x) for x in velocity], dtype=f32)
        self.angular_velocity = np.array([f32(x) for x in angular_velocity], dtype=f32)
        return self

    def motion(self):
        """the arguments of FluidSimulation3D.set_body_motion after the slot"""
        return self.centre, self.rot, self.velocity, self.angular_velocity


def apply_body(records, body, size, damping):
    """B(records): (new records, particles hit, particles re-clamped after their push).  `size`: the settings' box, `damping`: the
    tick's damping_factor."""
    field = body.field
    D, H, W = field.shape[:3]
    out = records.copy()
    p = out["position"].astype(f32)
    v = out["velocity"].astype(f32)
    b = np.array([f32(s) for s in size], dtype=f32) * f32(0.5)
    damping = f32(damping)
    c, r, u, w, ext = body.centre, body.rot, body.velocity, body.angular_velocity, body.extent
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = (f32(x) for x in r)
    with np.errstate(all="ignore"):
        hb = ext * f32(0.5)
        dx = p[:, 0] - c[0]
        dy = p[:, 1] - c[1]
        dz = p[:, 2] - c[2]
        qx = (r00 * dx + r10 * dy) + r20 * dz
        qy = (r01 * dx + r11 * dy) + r21 * dz
        qz = (r02 * dx + r12 * dy) + r22 * dz
        inside = (np.abs(qx) <= hb[0]) & (np.abs(qy) <= hb[1]) & (np.abs(qz) <= hb[2])
        idx = []
        for a, (q, wa) in enumerate(((qx, W), (qy, H), (qz, D))):
            x = q + hb[a]
            x = x / ext[a]
            x = x * f32(wa)
            idx.append(np.minimum(CR.u32_sat(x), np.uint64(wa - 1)).astype(np.int64))
        g = field[idx[2], idx[1], idx[0]]
        nz = (g[:, 0] != 0) | (g[:, 1] != 0) | (g[:, 2] != 0)
        ln = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        hit = inside & nz & (ln > f32(0))
        g, ln, ph, vh = g[hit], ln[hit], p[hit], v[hit]
        fx = (r00 * g[:, 0] + r01 * g[:, 1]) + r02 * g[:, 2]
        fy = (r10 * g[:, 0] + r11 * g[:, 1]) + r12 * g[:, 2]
        fz = (r20 * g[:, 0] + r21 * g[:, 1]) + r22 * g[:, 2]
        nx = fx / ln
        ny = fy / ln
        nz_ = fz / ln
        px = ph[:, 0] + fx
        py = ph[:, 1] + fy
        pz = ph[:, 2] + fz
        sx = px - c[0]
        sy = py - c[1]
        sz = pz - c[2]
        usx = u[0] + (w[1] * sz - w[2] * sy)
        usy = u[1] + (w[2] * sx - w[0] * sz)
        usz = u[2] + (w[0] * sy - w[1] * sx)
        rx = vh[:, 0] - usx
        ry = vh[:, 1] - usy
        rz = vh[:, 2] - usz
        rn = (rx * nx + ry * ny) + rz * nz_
        k = (f32(1.0) - damping) * rn
        vx = usx + (rx - k * nx)
        vy = usy + (ry - k * ny)
        vz = usz + (rz - k * nz_)
        ph = np.stack([px, py, pz], axis=1).astype(f32).reshape(-1, 3)
        vh = np.stack([vx, vy, vz], axis=1).astype(f32).reshape(-1, 3)
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


def apply_bodies(records, bodies, size, damping):
    """B_last(... B_first(records)) in the order given: (new records, hits per body, re-clamps per body)"""
    hits, clamps = [], []
    for body in bodies:
        records, h, c = apply_body(records, body, size, damping)
        hits.append(h)
        clamps.append(c)
    return records, hits, clamps


# ---- the shared scene: a paddle, a stirrer and a floor slab in dam_break_3d ------------------------------------------------
def solid_except(shape_dhw, axis, free):
    """a mask that is solid (255) except the slices `free` along `axis` (0: z, 1: y, 2: x)"""
    m = np.full(shape_dhw, 255, dtype=np.uint8)
    sl = [slice(None)] * 3
    for f in free:
        sl[axis] = f
        m[tuple(sl)] = 0
    return m


class Scene:
    """The three bodies of dam_break_3d(side^3) and their motion per step.  Slot order: paddle, stirrer, floor slab."""

    def __init__(self, fs, side):
        st, off, tick = fs.dam_break_3d(side ** 3)
        self.fs, self.st, self.off, self.tick = fs, st, off, tick
        self.size = (st.size.x, st.size.y, st.size.z)
        sx, sy, sz = (float(s) for s in self.size)
        L = side * 0.1
        self.dt = f32(tick.delta)
        self.masks = [solid_except((4, 4, 8), 2, (0, -1)), solid_except((2, 5, 10), 1, (0, -1)), solid_except((1, 6, 4), 1, (-1,))]
        self.extents = [(0.3, sy, sz), (1.2, 0.3, sz), (0.8, 0.6, sz)]
        self.paddle_u = np.array([-1.5, 0.0, 0.0], dtype=f32)
        self.paddle_c0 = np.array([-sx / 2 + L + 0.1, 0.0, 0.0], dtype=f32)
        self.stirrer_c = (-sx / 2 + 0.5 * L, sy / 2 - 0.5, 0.0)
        self.slab_c = (-sx / 2 + 0.5 * L, sy / 2, 0.0)
        self.slab_rot = fs.rigid_motion(self.slab_c, (0, 0, 0), (1, 0, 0), 0.3, 1.0)[1]
        self.fields = [CR.producer_field(m, e) for m, e in zip(self.masks, self.extents)]

    def bodies(self):
        """fresh Body objects, motion not yet set"""
        return [Body(f, e) for f, e in zip(self.fields, self.extents)]

    def set_motions(self, bodies, s):
        """the motion of step s = 1, 2, ... into `bodies`: the paddle's centre is advanced by u * dt in f32 once per step (step 1
        starts from the start position), the stirrer is turned by 4 * s * dt about z, the slab rests"""
        c = self.paddle_c0.copy()
        for _ in range(s - 1):
            c = c + self.paddle_u * self.dt
        bodies[0].set_motion(c, IDENTITY, self.paddle_u)
        sc, srot = self.fs.rigid_motion(self.stirrer_c, (0, 0, 0), (0, 0, 1), 4.0, float(s) * float(self.dt))
        bodies[1].set_motion(sc, srot, (0, 0, 0), (0.0, 0.0, 4.0))
        bodies[2].set_motion(self.slab_c, self.slab_rot)
        return bodies


_RUNS = {}


def oracle_run(fs, orc, side, static=None, steps=40, keep=(1, 8, 40)):
    """The scene on the CPU: the unchanged 3D oracle, then C of §18's scene `static` ('a' or None), then the three operators,
    applied to its records after every step.  {"snap": {step: records}, "hits": per-body hits per step [steps, 3], "reclamped":
    likewise, "scene": Scene, "static": field or None}; computed once, never changed."""
    key = (side, static, steps, tuple(keep))
    if key not in _RUNS:
        sc = Scene(fs, side)
        field = CR.scene_box_on_floor(sc.size) if static == "a" else None
        bodies = sc.bodies()
        ref = orc.OracleSim3D(sc.st, initial_offset=sc.off)
        snap, hits, clamps = {}, [], []
        for s in range(1, steps + 1):
            ref.step(sc.tick)
            rec = ref.particles()
            if field is not None:
                rec = CR.apply_collider(rec, field, sc.size, sc.tick.damping_factor)[0]
            rec, h, c = apply_bodies(rec, sc.set_motions(bodies, s), sc.size, sc.tick.damping_factor)
            ref.set_particles(rec)
            hits.append(h)
            clamps.append(c)
            if s in keep:
                snap[s] = rec
        ref.close()
        for r in snap.values():
            r.setflags(write=False)
        _RUNS[key] = {"snap": snap, "hits": np.array(hits), "reclamped": np.array(clamps), "scene": sc, "static": field}
    return _RUNS[key]
