"""The 3D moving bodies and their loads (include/fluidsim.h "3D moving bodies", "3D body loads") at the hard
inputs of the plain 3D step and at the operator's own operand guards: the 3D form of tests/body_cases2d.py, whose text explains
the bodies and the guards.  One registry for tests/test_bodies3d_hard_inputs_gpu.py and for the CPU companion
tests/test_bodies_hard_inputs.py.  TEST INFRASTRUCTURE ONLY, no GPU.

What differs from 2D: the reference is the unchanged oracle.OracleSim3D with body_loads3d_ref.apply_bodies after every step (no
sort modes, no start indices); the cover field is 5 x 4 x 3, the spinner turns about two axes; besides the edge body (1024 x 1 x 1,
one particle exactly on its +x face, reading voxel 1023 through the clamp) a second one, `edge-z` (1 x 1 x 4), holds another
particle exactly on its -z face, reading voxel 0; the whirl spins about two axes in the families guard, faces and wall.  The
kernels take one particle per lane: of PLANT, 63 | 64 is a wave seam and 511 | 512 a workgroup seam."""
import numpy as np

from tests import bodies3d_ref as B
from tests import body_loads3d_ref as L
from tests import collide3d_ref as CR
from tests import hard_states3d as H
from tests.body_cases2d import (EDGE_HB, EDGE_W, MID, PLANT, SMALL, BodyRun, Guard, Step, _check_entry, _check_zero_rot, _no_hit,  # noqa: F401
                                 copy_tick, expect, finite_rows, flush, has_nan, makers_and_target)

f32 = np.float32
NAMES = ("cover", "spinner", "edge", "edge-z", "whirl")
WHIRL_FAMILIES = ("guard", "faces", "wall")
COVER_SHAPE, SPINNER_SHAPE = (5, 4, 3), (4, 3, 2)
EDGE_Z_D = 4
WHIRL_EXTENT = (3.0, 3.0, 3.0)
WHIRL_OFFSET = np.array([1.3, -1.3, 1.3], dtype=f32)


def rot3(theta, phi):
    """row-major R = Rz(theta) Rx(phi): float64, cast to float32 once"""
    c, s, d, t = np.cos(theta), np.sin(theta), np.cos(phi), np.sin(phi)
    rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)
    rx = np.array([[1, 0, 0], [0, d, -t], [0, t, d]], dtype=np.float64)
    return (rz @ rx).reshape(9).astype(f32)


def frozen(body):
    return B.Body(body.field, body.extent, *body.motion())


def voxels(body, pos):
    """(ix, iy, iz, inside) of every position by the header's lines, f32, this association"""
    c, ext = body.centre, body.extent
    r00, r01, r02, r10, r11, r12, r20, r21, r22 = (f32(x) for x in body.rot)
    D_, H_, W_ = body.field.shape[:3]
    pos = np.asarray(pos, dtype=f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        hb = ext * f32(0.5)
        dx = pos[:, 0] - c[0]
        dy = pos[:, 1] - c[1]
        dz = pos[:, 2] - c[2]
        qx = (r00 * dx + r10 * dy) + r20 * dz
        qy = (r01 * dx + r11 * dy) + r21 * dz
        qz = (r02 * dx + r12 * dy) + r22 * dz
        inside = (np.abs(qx) <= hb[0]) & (np.abs(qy) <= hb[1]) & (np.abs(qz) <= hb[2])
        out = []
        for a, (q, wa) in enumerate(((qx, W_), (qy, H_), (qz, D_))):
            x = q + hb[a]
            x = x / ext[a]
            x = x * f32(wa)
            out.append(np.minimum(CR.u32_sat(x), np.uint64(wa - 1)).astype(np.int64))
    return out[0], out[1], out[2], inside


def on_edge_reads_last_pixel(body, p):
    """the edge body (W = 1024): the particle lies exactly on its +x face (p.x - c.x == hb.x in f32), its voxel expression reaches
    W and it reads voxel W - 1.  The edge-z body: the particle lies exactly on its -z face (p.z - c.z == -hb.z) and reads voxel 0."""
    p = np.asarray(p, dtype=f32)
    ix, iy, iz, inside = voxels(body, p)
    ok = bool(inside[0]) and tuple(body.rot) == B.IDENTITY
    if body.field.shape[2] == EDGE_W:
        hb = body.extent[0] * f32(0.5)
        q = p[0] - body.centre[0]
        raw = ((q + hb) / body.extent[0]) * f32(EDGE_W)
        return ok and bool(q == hb and raw >= f32(EDGE_W) and ix[0] == EDGE_W - 1)
    hb = body.extent[2] * f32(0.5)
    q = p[2] - body.centre[2]
    return ok and bool(q == -hb and (q + hb) == 0 and iz[0] == 0)


# ---- a. the registry with bodies --------------------------------------------------------------------------------------------
def _cover_field(first, size, h, seed):
    """body_cases2d._cover_field in 3D: 5 x 4 x 3 without a free voxel; where the first state keeps more than 0.25 h from every
    wall, the voxel of the particle nearest a wall pushes straight at that wall by 1.25 times its distance"""
    f = CR.random_field(COVER_SHAPE, seed, fill=1.0, mag=0.25 * h)
    pos = first["position"][finite_rows(first["position"])].astype(np.float64)
    gap = np.array(size, dtype=np.float64) * 0.5 - np.abs(pos)
    if pos.shape[0] and gap.min() > 0.25 * h:
        j, a = np.unravel_index(np.argmin(gap), gap.shape)
        ix, iy, iz, _ = voxels(B.Body(f, tuple(2.0 * x for x in size)), pos[j])
        v = np.zeros(3)
        v[a] = (1.0 if pos[j, a] >= 0 else -1.0) * 1.25 * gap[j, a]
        f[iz[0], iy[0], ix[0]] = v
    return f


def _edge_field(h):
    f = CR.random_field((EDGE_W, 1, 1), 1024, fill=0.5, mag=0.1 * h)
    f[0, 0, EDGE_W - 2] = (-0.25 * h, -0.125 * h, 0.1 * h)
    f[0, 0, EDGE_W - 1] = (0.0, 2.0 * h, 0.0)
    return f


def _edge_z_field(h):
    f = np.zeros((EDGE_Z_D, 1, 1, 3), dtype=f32)
    f[:, 0, 0] = [(0.0, 0.1 * h, -2.0 * h), (0.2 * h, 0.0, 0.0), (0.0, -0.2 * h, 0.0), (0.1 * h, 0.1 * h, 0.1 * h)]
    return f


def _whirl_field(h):
    """8^3 voxels over 3^3 units, two push: the corner voxel that holds the particle the body is placed by (3e38 * s
    overflows there: NaN), and a voxel beside the centre (finite and enormous)"""
    f = np.zeros((8, 8, 8, 3), dtype=f32)
    f[0, 7, 0] = (0.0, 0.15 * h, 0.0)
    f[3, 4, 3] = (0.1 * h, -0.05 * h, 0.05 * h)
    return f


def _edge_centre(rec, hb, axis, sign, skip=None):
    """(particle, centre) with p.a - c.a == sign * hb exactly in f32, or None; the finite particles in descending y (the floor first)"""
    pos = rec["position"]
    hb = f32(hb)
    ok = np.flatnonzero(finite_rows(pos))
    for j in ok[np.argsort(-pos[ok, 1], kind="stable")][:64]:
        if j == skip:
            continue
        ca = f32(pos[j, axis] - f32(sign) * hb)
        if f32(pos[j, axis] - ca) == f32(sign) * hb:
            c = pos[j].copy()
            c[axis] = ca
            return int(j), c
    return None


def _run_with(case, hb):
    st, tick = case.st, case.tick
    h = float(st.smoothing_radius)
    size = (st.size.x, st.size.y, st.size.z)
    damping = tick.damping_factor
    whirl = case.name.split("/")[0] in WHIRL_FAMILIES
    seed = sum(case.name.encode()) % 1000
    cube = (2.0 * hb,) * 3
    bodies = [B.Body(_cover_field(case.run()[0], size, h, seed), tuple(2.0 * s for s in size)),
              B.Body(CR.random_field(SPINNER_SHAPE, seed + 1, fill=1.0, mag=0.2 * h), (5.0 * h, 3.0 * h, 4.0 * h)),
              B.Body(_edge_field(h), cube), B.Body(_edge_z_field(h), cube)]
    if whirl:
        bodies.append(B.Body(_whirl_field(h), WHIRL_EXTENT))
    ref = case.orc.OracleSim3D(st, case.off)
    ref.set_particles(case.start)
    acc = [L.ZERO] * len(bodies)
    steps, missed = [], False
    none = np.zeros(0, dtype=np.uint32)
    with np.errstate(all="ignore"):
        for s in range(1, case.steps + 1):
            ref.step(tick)
            before = ref.particles()
            met = B.apply_body(before, bodies[0], size, damping)[0]            # the median of what the cover leaves
            ok = finite_rows(met["position"])
            if ok.any():
                pos = met["position"][ok].astype(np.float64)
                med = met["position"][ok][np.argmin(((pos - np.median(pos, axis=0)) ** 2).sum(axis=1))]     # the particle nearest the median
                bodies[1].set_motion(med, rot3(0.3 + 0.7 * s, 0.2 * s), (4.0 * h, -2.5 * h, 1.5 * h), (0.5, -1.0, 2.0))
                if whirl:
                    bodies[4].set_motion(med + WHIRL_OFFSET, B.IDENTITY, (0.0, 0.0, 0.0), (0.0, 3e38, 3e38))
            met_x = B.apply_bodies(before, bodies[:2], size, damping)[0]
            fx = _edge_centre(met_x, hb, 0, 1.0)
            if fx:
                bodies[2].set_motion(fx[1])
            met_z = B.apply_body(met_x, bodies[2], size, damping)[0]
            fz = _edge_centre(met_z, hb, 2, -1.0, skip=fx[0] if fx else None)
            if fz:
                bodies[3].set_motion(fz[1])
            missed |= (fx is None and finite_rows(met_x["position"]).any()) or (fz is None and finite_rows(met_z["position"]).sum() > 1)
            rec, words, recs = L.apply_bodies(before, bodies, size, damping)
            ref.set_particles(rec)
            acc = [L.add_words(a, w) for a, w in zip(acc, words)]
            steps.append(Step3(before, rec, none.copy(), [frozen(b) for b in bodies], words, recs, acc,
                               [fx[0] if fx else None, fz[0] if fz else None], {2: met_x, 3: met_z}))
    ref.close()
    return BodyRun(case, NAMES[:len(bodies)], [b.field for b in bodies], [b.extent for b in bodies], steps, hb), missed


class Step3(Step):
    def hits(self):
        return [w[6] for w in self.words]

    def dropped(self):
        return [w[7] for w in self.words]


_RUNS = {}


def registry_run(fs, orc, cid):
    """the case `cid` of hard_states3d with bodies, computed once: the first hb of EDGE_HB with which every step finds its two
    edge particles"""
    if cid not in _RUNS:
        case = H.case_by_id(fs, orc, cid)
        for hb in EDGE_HB:
            run, missed = _run_with(case, hb)
            if not missed:
                break
        assert not missed, f"{cid}: no hb of EDGE_HB gives every step its edge particles"
        _RUNS[cid] = run
    return _RUNS[cid]


CASE_IDS = list(H.CASE_IDS)
WHIRL_IDS = [c for c in CASE_IDS if c.split("/")[0] in WHIRL_FAMILIES]


def describe(run):
    c = run.case
    return (f"[body_cases3d] {c.name} (n {c.n}, hb {run.hb}): hits {[s.hits() for s in run.steps]}, re-clamped "
            f"{[s.reclamped() for s in run.steps]}, dropped {[s.dropped() for s in run.steps]}, edge {[s.edge for s in run.steps]}, "
            f"NaN after {[int(s.nan) for s in run.steps]}")


# ---- b. the operator's own guards -------------------------------------------------------------------------------------------
GUARD_N, GUARD_SEED = 4097, 31
PICK_RES = 96


def guard_base(fs, orc):
    """(settings, offset, tick, records): 4097 particles of the oracle's lattice in a 4 x 3 x 2.5 box, jittered"""
    st = fs.Settings3(GUARD_N, 0.1, 0.2, fs.Vec3(4.0, 3.0, 2.5))
    tick = fs.TickSettings3(float(f32(1) / f32(120)), fs.Vec3(0.3, 9.81, -0.2), 1.0, 50.0, 0.0, 0.1, 25.0)
    off = (0.0, 0.0, 0.0)
    ref = orc.OracleSim3D(st, off)
    p = ref.particles()
    ref.close()
    rng = np.random.default_rng(GUARD_SEED)
    p["position"] += rng.uniform(-0.025, 0.025, size=(GUARD_N, 3)).astype(f32)
    p["velocity"] = rng.uniform(-1.0, 1.0, size=(GUARD_N, 3)).astype(f32)
    p["predicted_position"] = p["position"]
    return st, off, tick, p


def guard_engine_settings(fs):
    """the engine takes a cube count at create: the guard handles are created with 16^3 particles, given room (GUARD_CAPACITY)
    and receive the first 4096 records by upload and the last one by emit"""
    return fs.Settings3(GUARD_N - 1, 0.1, 0.2, fs.Vec3(4.0, 3.0, 2.5))


GUARD_CAPACITY = 4200


def picker(pos, slots, vector, **motion):
    """a body over the bounding box of the finite positions (PICK_RES^3 voxels, identity rotation) whose field holds `vector` in
    the voxels of the particles `slots` and nothing elsewhere"""
    ok = finite_rows(pos)
    lo, hi = pos[ok].min(axis=0).astype(np.float64) - 0.01, pos[ok].max(axis=0).astype(np.float64) + 0.01
    body = B.Body(np.zeros((PICK_RES, PICK_RES, PICK_RES, 3), dtype=f32), hi - lo, centre=(lo + hi) / 2, **motion)
    ix, iy, iz, inside = voxels(body, pos[list(slots)])
    assert inside.all()
    body.field[iz, iy, ix] = vector
    return body


def hit_slots(rec):
    return [int(i) for i in np.flatnonzero(rec["hit"])]


class Guard3(Guard):
    def reference(self, after, size, tick):
        bodies = self.bodies(after, size)
        want, words, recs = L.apply_bodies(after, bodies, size, tick.damping_factor)
        return bodies, want, words, recs


def _small_velocities(p):
    pool = np.array(SMALL, dtype=f32)
    p["velocity"] = pool[np.random.default_rng(3).integers(0, pool.size, size=p["velocity"].shape)]
    return p


def _makers_and_target(after, size):
    """body_cases2d.makers_and_target with the spin about z, so that us.z = u.z stays finite"""
    return makers_and_target(after, size, B.apply_body, picker, [(6e-4, 8e-4, 3e-4), (1e-3, 0.0, 0.0), (-3e-4, 4e-4, 1e-4)],
                             dict(velocity=(3e38, -3e38, 3e38), angular_velocity=(0.0, 0.0, -3e38)),
                             dict(velocity=(-3e38, 3e38, -3e38), angular_velocity=(0.0, 0.0, -3e38)),
                             dict(velocity=(3.38e38, -3e38, 1e38)),
                             dict(velocity=(0.5, 0.25, -0.5), angular_velocity=(1.0, 0.5, -1.0)), np.array([-0.5, 0.6, 0.0]))


def _positions(p):
    kinds = [(0, np.nan), (2, np.nan), (0, np.inf), (1, -np.inf), (2, np.inf)]
    for k, slot in enumerate(PLANT):
        a, x = kinds[k % len(kinds)]
        p["position"][slot, a] = x
    p["predicted_position"] = p["position"]
    return p


def _cover(size, field, **motion):
    return B.Body(np.asarray(field, dtype=f32), tuple(2.0 * s for s in size), **motion)


def _one(vector):
    return np.array(vector, dtype=f32).reshape(1, 1, 1, 3)


def _centred(after, slot=MID):
    return after["position"][slot]


def _check_positions(after, want, words, recs):
    nan = np.isnan(after["position"]).any(axis=1)
    assert nan.sum() >= 4 and np.isfinite(after["position"][~nan]).all(), "the step leaves a NaN position and clamps an infinite one"
    expect("one", "none", "none", 0, MID)(after, want, words, recs)    # the particle exactly at the centre of the first body
    assert words[1][6] == int((~nan).sum()) and not recs[1]["hit"][nan].any(), "NaN: outside; every finite particle: inside"
    assert words[1][7] == 0 and 0 < int(recs[1]["clamped"].sum()) < words[1][6], "the cover: no drop, some re-clamps"
    assert want["position"][nan].tobytes() == after["position"][nan].tobytes() and want["velocity"][nan].tobytes() == after["velocity"][nan].tobytes()
    return f"NaN positions {int(nan.sum())}, hits {[w[6] for w in words]}"


FOUR = np.array([[[[0.01, 0.0, 0.0], [0.0, 0.02, 0.0], [-0.03, 0.0, 0.0], [0.0, 0.0, -0.04]]]], dtype=f32)     # 4 x 1 x 1


def denormal_extent_body(after):
    return B.Body(FOUR, (1e-40, 1.0, 1.0), centre=_centred(after))


def _check_denormal_extent(after, want, words, recs):
    """(0 + hb) / extent = 0.5 from two denormals: voxel 2; with the operands flushed, 0 / 0 is a NaN and the voxel is 0"""
    body = denormal_extent_body(after)
    ix = voxels(body, after["position"][MID])[0][0]
    with np.errstate(all="ignore"):
        flushed = (flush(body.extent * f32(0.5))[0] / flush(body.extent)[0]) * f32(4)
    other = int(min(CR.u32_sat(flushed), 3))
    expect("one", "none", "none", 0, MID)(after, want, words, recs)
    assert ix == 2 and other != 2, (ix, other)
    moved = want["position"][MID] - after["position"][MID]
    assert moved[0] < 0 and moved[1] == 0 and moved[2] == 0, "the vector of voxel 2"
    return f"voxel {ix}, a flushed quotient gives voxel {other}"


def _eight(after, size):
    """eight bodies, each centred where the one before left the last particle: through the ceiling, through the floor, ..."""
    out, rec = [], after
    with np.errstate(all="ignore"):
        for k in range(8):
            body = B.Body(_one((0.0, (-2.0 if k % 2 == 0 else 2.0) * size[1], 0.0)), (0.02, 0.02, 0.02), centre=rec["position"][4096],
                          velocity=(0.1 * k, -0.2, 0.1), angular_velocity=(0.5 * k, 0.0, -0.25))
            rec = B.apply_body(rec, body, size, 0.1)[0]               # (positions: whatever the damping)
            out.append(body)
    return out


def _check_eight(after, want, words, recs):
    for k in range(8):                                                 # the last particle: eight hits, eight re-clamps, no drop
        expect("one", "none", "all", k, after.shape[0] - 1)(after, want, words, recs)
    return f"hits {[w[6] for w in words]}"


def _through_floor(after, size):
    return [_cover(size, _one((0.0, 2.0 * size[1], 0.0)), velocity=(0.3, -0.2, 0.1), angular_velocity=(0.5, 0.0, 0.25))]


def _guards():
    c = lambda f: (lambda after, size: [f(after, size)])               # noqa: E731
    cover = lambda field, **m: c(lambda after, size: _cover(size, field, **m))      # noqa: E731
    at = lambda field, extent, **m: c(lambda after, size: B.Body(field, extent, centre=_centred(after), **m))      # noqa: E731
    wide = CR.random_field((4, 3, 3), 9, fill=1.0, mag=0.05)
    big = 1e38
    out = [
        Guard3("entry_velocities", _makers_and_target, _check_entry, state=_small_velocities, delta=0.0, gravity=(-1.0, -9.81, -0.5)),
        Guard3("positions", lambda after, size: [B.Body(_one((0.01, 0.02, -0.01)), (1e-4, 1e-4, 1e-4), centre=_centred(after)), _cover(size, wide)],
               _check_positions, state=_positions),
        Guard3("rot/zero", at(wide, (1.0, 1.0, 1.0), rot=(0.0,) * 9, velocity=(0.2, 0.1, -0.1), angular_velocity=(1.0, 0.0, 0.5)), _check_zero_rot),
        Guard3("rot/tenth", at(wide, (0.1, 0.1, 0.1), rot=(0.1, 0.0, 0.0, 0.0, 0.1, 0.0, 0.0, 0.0, 0.1)), expect("some", "none", "none")),
        Guard3("rot/1e38", at(wide, (1.0, 1.0, 1.0), rot=(big, big, 0.0, -big, big, 0.0, 0.0, big, big)), expect("one", "all", "all", 0, MID)),
        Guard3("rot/reflection", at(wide, (1.0, 0.8, 0.6), rot=(1.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 1.0), angular_velocity=(0.0, 0.0, 1.0)), expect("some", "none", "none")),
        Guard3("extent/2^-149", at(wide, (2.0 ** -149, 1.0, 1.0)), expect("one", "none", "none", 0, MID)),
        Guard3("extent/1e-40", lambda after, size: [denormal_extent_body(after)], _check_denormal_extent),
        Guard3("extent/1e30", at(wide, (1e30, 1e30, 1e30)), expect("all", "none", "none")),
        Guard3("extent/3e38", at(wide, (3e38, 3e38, 3e38)), expect("all", "none", "none")),
        Guard3("field/3e38", cover(_one((3e38, 1e30, -3e38))), expect("all", "none", "all")),
        Guard3("field/1e30", cover(_one((-1e30, 1e30, 1e30)), velocity=(0.5, 0.5, 0.5)), expect("all", "some", "all")),
        Guard3("field/-0", cover(_one((-0.0, 0.0, -0.0))), _no_hit),
        Guard3("field/half_underflow", cover(_one((1e-40, 1e-19, 1e-30))), expect("all", "none", "none")),
        Guard3("field/underflow", cover(_one((1e-30, 1e-30, 1e-30))), _no_hit),
        Guard3("motion/3e38", cover(wide, velocity=(3e38, -3e38, 3e38), angular_velocity=(-3e38, 0.0, -3e38)), expect("all", "all", "none")),
        Guard3("eight_on_one", _eight, _check_eight),
    ]
    out += [Guard3(f"damping/{d}", _through_floor, expect("all", "none", "all"), damping_factor=d) for d in (0.0, 1.0, 1.5, -0.5)]
    return out


GUARDS = {g.name: g for g in _guards()}
GUARD_IDS = list(GUARDS)
MODE_GUARD = "entry_velocities"                                        # the guard that also runs in FS_MATH_TOLERANCE
