"""The 2D moving bodies and their loads (include/fluidsim.h "2D moving bodies", "2D body loads") at the hard
inputs of the plain 2D step and at the operator's own operand guards: the cases, chosen on the CPU alone.  One registry for
tests/test_bodies2d_hard_inputs_gpu.py (the engine against the reference) and for the CPU companion
tests/test_bodies_hard_inputs.py (the reference alone: the cases test what they say).  TEST INFRASTRUCTURE ONLY, no GPU.

a. Every case of tests/hard_states2d.CASE_IDS with bodies (`registry_run`).  The reference is that of bodies2d_ref.oracle_run:
   the unchanged oracle as hard_states2d.Case.checker sets it up (quirks, sort mode, field, start indices), after every step the
   operators in slot order through body_loads2d_ref.apply_bodies, then set_particles with the result.  The poses of a step are
   derived from the reference state of that step, so that they hit it whatever the case's box, offset and radius are:
     cover    identity pose at the origin, extent twice the box, a 7 x 5 field without a free pixel: every finite particle is
              hit in every step, and its pushes carry particles through the walls (_cover_field: also where the fluid keeps
              far from every wall)
     spinner  turned, translating and spinning, 5 h x 3 h, centred on the particle nearest the median finite position of the step's
              records as the cover leaves them
     edge     identity rotation, 1024 x 1 pixels with distinct vectors in the last two; its centre is chosen per step so that one
              particle of the state it meets (after cover and spinner) has p.x - c.x == hb.x exactly in f32: "on an edge:
              inside", and the pixel index 1024 is clamped to 1023
     whirl    (families guard, nan_clamp, coincident, dam) angular velocity 3e38: its hits are dropped as out of range or NaN
              and it leaves NaN and enormous velocities for the next plain step
b. The operator's own guards (`GUARDS`): one step of a jittered 4097-particle block, the reference is apply_bodies on what a
   body-less step leaves.  The plain step hands every operator a finite velocity of at most 500 and a position that is finite or
   NaN (it zeroes a NaN velocity, clamps the speed and clamps an infinite position onto a wall), so NaN, infinite and enormous
   ENTRY velocities are made by earlier bodies (makers_and_target: velocity +-3e38, angular velocity -3e38) for a later one.  The particles the
   guards aim at are those of PLANT, slots of the array the bodies' kernels read: both halves of a lane's pair, pairs of which
   one half is hit, the wave and workgroup seams, and the last particle of the odd count.  A `picker` body — a fine field over
   the fluid's bounding box with a vector only in the pixels of the wanted particles — hits exactly these.  Every guard's check
   asserts its hits, its dropped hits and its re-clamps (`expect`).
c. The loads' shard table over more than 64 workgroups (`MANY_WORKGROUPS`)."""
import numpy as np

from tests import bodies2d_ref as B
from tests import body_loads2d_ref as L
from tests import collide3d_ref as CR
from tests import hard_states2d as H
from tests import parity_states as PS

f32 = np.float32
NAMES = ("cover", "spinner", "edge", "whirl")
WHIRL_FAMILIES = ("guard", "nan_clamp", "coincident", "dam")
EDGE_W = 1024
EDGE_HB = (0.75, 0.5, 1.0, 0.375, 0.625, 0.25, 1.5, 0.125)
COVER_SHAPE, SPINNER_SHAPE = (7, 5), (5, 4)


def rot2(theta):
    """row-major R of a counter-clockwise turn by theta: float64, cast to float32 once (as rigid_motion2d)"""
    return np.array([np.cos(theta), -np.sin(theta), np.sin(theta), np.cos(theta)], dtype=np.float64).astype(f32)


def frozen(body):
    """a copy of a body with its present motion"""
    return B.Body(body.field, body.extent, *body.motion())


def pixels(body, pos):
    """(ix, iy, inside) of every position by the header's lines, f32, one operation per line — restated here so that the cases can
    say which pixel a particle reads"""
    c, ext = body.centre, body.extent
    r00, r01, r10, r11 = (f32(x) for x in body.rot)
    H_, W_ = body.field.shape[:2]
    pos = np.asarray(pos, dtype=f32).reshape(-1, 2)
    with np.errstate(all="ignore"):
        hb = ext * f32(0.5)
        dx = pos[:, 0] - c[0]
        dy = pos[:, 1] - c[1]
        t0 = r00 * dx
        t1 = r10 * dy
        qx = t0 + t1
        t0 = r01 * dx
        t1 = r11 * dy
        qy = t0 + t1
        inside = (np.abs(qx) <= hb[0]) & (np.abs(qy) <= hb[1])
        out = []
        for a, (q, wa) in enumerate(((qx, W_), (qy, H_))):
            x = q + hb[a]
            x = x / ext[a]
            x = x * f32(wa)
            out.append(np.minimum(CR.u32_sat(x), np.uint64(wa - 1)).astype(np.int64))
    return out[0], out[1], inside


def flush(x):
    """x with denormals flushed to zero, sign kept: what an f32 unit without denormal support reads and writes"""
    x = np.asarray(x, dtype=f32).copy()
    x[np.abs(x) < np.finfo(f32).tiny] *= f32(0)
    return x


def on_edge_reads_last_pixel(body, p):
    """the particle at p lies exactly on the +x edge of the body's box (p.x - c.x == hb.x in f32, identity rotation), its pixel
    expression reaches W and the index it reads is W - 1"""
    W_ = body.field.shape[1]
    p = np.asarray(p, dtype=f32)
    hb = body.extent[0] * f32(0.5)
    q = p[0] - body.centre[0]
    raw = ((q + hb) / body.extent[0]) * f32(W_)
    ix, _, inside = pixels(body, p)
    return bool(q == hb and raw >= f32(W_) and inside[0] and ix[0] == W_ - 1 and tuple(body.rot) == B.IDENTITY)


def finite_rows(pos):
    return np.isfinite(pos).all(axis=1)


def has_nan(rec):
    return bool(any(np.isnan(rec[f]).any() for f in H.FLOAT_FIELDS))


# ---- a. the registry with bodies --------------------------------------------------------------------------------------------
class Step:
    """one reference step of a case: `before` (the oracle's records before the bodies), `rec` and `start` after them, `bodies`
    (frozen, slot order: the poses the handle is given before this step), per body the step's `words` and per-hit `recs`, `acc`
    (the words accumulated over the steps so far), `edge` (per edge body: its particle or None) and `edge_before` ({slot of an
    edge body: the records it met})"""

    def __init__(self, before, rec, start, bodies, words, recs, acc, edge, edge_before):
        self.before, self.rec, self.start, self.bodies, self.words, self.recs, self.acc = before, rec, start, bodies, words, recs, acc
        self.edge, self.edge_before = edge, edge_before
        self.nan = has_nan(rec)
        for a in (before, rec, start):
            a.setflags(write=False)

    def hits(self):
        return [w[3] for w in self.words]

    def dropped(self):
        return [w[4] for w in self.words]

    def reclamped(self):
        return [int(r["clamped"].sum()) for r in self.recs]


class BodyRun:
    def __init__(self, case, names, fields, extents, steps, hb):
        self.case, self.names, self.fields, self.extents, self.steps, self.hb = case, names, fields, extents, steps, hb


def _cover_field(first, size, h, seed):
    """7 x 5 without a free pixel, components up to 0.25 h.  Where the state the cover first meets (`first`: the plain oracle's
    records after step 1) keeps more than 0.25 h from every wall, no such push reaches one: the pixel of the particle nearest a
    wall then pushes straight at that wall by 1.25 times the particle's distance from it"""
    f = B.random_field(COVER_SHAPE, seed, fill=1.0, mag=0.25 * h)
    pos = first["position"][finite_rows(first["position"])].astype(np.float64)
    gap = np.array(size, dtype=np.float64) * 0.5 - np.abs(pos)
    if pos.shape[0] and gap.min() > 0.25 * h:
        j, a = np.unravel_index(np.argmin(gap), gap.shape)
        ix, iy, _ = pixels(B.Body(f, (2.0 * size[0], 2.0 * size[1])), pos[j])
        v = np.zeros(2)
        v[a] = (1.0 if pos[j, a] >= 0 else -1.0) * 1.25 * gap[j, a]
        f[iy[0], ix[0]] = v
    return f


def _edge_field(h):
    """1024 x 1: half of the pixels push a little, the last two push differently from each other — (0, 2 h) in pixel W - 1, which
    the edge particle reads through the clamp, so that a particle on the floor is pushed through it"""
    f = B.random_field((EDGE_W, 1), 1024, fill=0.5, mag=0.1 * h)
    f[0, EDGE_W - 2] = (-0.25 * h, -0.125 * h)
    f[0, EDGE_W - 1] = (0.0, 2.0 * h)
    return f


WHIRL_EXTENT = (3.0, 3.0)
WHIRL_OFFSET = np.array([1.3, -1.3], dtype=f32)


def _whirl_field(h):
    """8 x 8 over 3 x 3 units, two pixels push: the corner pixel that holds the particle the body is placed by, at
    s = (-1.3, 1.3) from the centre, where 3e38 * s overflows and inf - inf makes the velocity a NaN; and a pixel beside the
    centre, where the surface velocity is finite and enormous"""
    f = np.zeros((8, 8, 2), dtype=f32)
    f[7, 0] = (0.0, 0.15 * h)
    f[4, 3] = (0.1 * h, -0.05 * h)
    return f


def _edge_centre(rec, hb):
    """(particle, centre) with p.x - c.x == hb exactly in f32, or None: the finite particles in descending y (the floor first),
    c.x = p.x - hb rounded once"""
    pos = rec["position"]
    hb = f32(hb)
    ok = np.flatnonzero(finite_rows(pos))
    for j in ok[np.argsort(-pos[ok, 1], kind="stable")][:64]:
        cx = f32(pos[j, 0] - hb)
        if f32(pos[j, 0] - cx) == hb:
            return int(j), (cx, pos[j, 1])
    return None


def _run_with(case, hb):
    st, tick = case.st, case.tick
    h = float(st.smoothing_radius)
    size = (st.size.x, st.size.y)
    damping = tick.damping_factor
    whirl = case.family in WHIRL_FAMILIES
    seed = sum(case.name.encode()) % 1000
    bodies = [B.Body(_cover_field(case.run()[0].rec, size, h, seed), (2.0 * size[0], 2.0 * size[1])),
              B.Body(B.random_field(SPINNER_SHAPE, seed + 1, fill=1.0, mag=0.2 * h), (5.0 * h, 3.0 * h)),
              B.Body(_edge_field(h), (2.0 * hb, 2.0 * hb))]
    if whirl:
        bodies.append(B.Body(_whirl_field(h), WHIRL_EXTENT))
    chk = case.checker()
    acc = [L.ZERO] * len(bodies)
    steps, missed = [], False
    with np.errstate(all="ignore"):
        for s in range(1, case.steps + 1):
            chk.step(tick, stable_sort=case.stable)
            before = chk.particles()
            met = B.apply_body(before, bodies[0], size, damping)[0]            # the median of what the cover leaves
            ok = finite_rows(met["position"])
            if ok.any():
                pos = met["position"][ok].astype(np.float64)
                med = met["position"][ok][np.argmin(((pos - np.median(pos, axis=0)) ** 2).sum(axis=1))]     # the particle nearest the median
                bodies[1].set_motion(med, rot2(0.3 + 0.7 * s), (4.0 * h, -2.5 * h), 2.0)
                if whirl:
                    bodies[3].set_motion(med + WHIRL_OFFSET, B.IDENTITY, (0.0, 0.0), 3e38)
            met = B.apply_bodies(before, bodies[:2], size, damping)[0]         # what the edge body meets
            found = _edge_centre(met, hb)
            if found:
                bodies[2].set_motion(found[1])
            elif finite_rows(met["position"]).any():
                missed = True
            rec, words, recs = L.apply_bodies(before, bodies, size, damping)
            chk.set_particles(rec)
            acc = [L.add_words(a, w) for a, w in zip(acc, words)]
            steps.append(Step(before, rec, chk.start_indices_view().copy(), [frozen(b) for b in bodies], words, recs, acc,
                              [found[0] if found else None], {2: met}))
    chk.close()
    return BodyRun(case, NAMES[:len(bodies)], [b.field for b in bodies], [b.extent for b in bodies], steps, hb), missed


_RUNS = {}


def registry_run(fs, orc, cid):
    """the case `cid` of hard_states2d with bodies, computed once: the first hb of EDGE_HB with which every step that has a finite
    position finds its edge particle"""
    if cid not in _RUNS:
        case = H.case_by_id(fs, orc, cid)
        case.run()                                                     # settles the upload order (hard_states2d.Case.run)
        for hb in EDGE_HB:
            run, missed = _run_with(case, hb)
            if not missed:
                break
        assert not missed, f"{cid}: no hb of EDGE_HB gives every step its edge particle"
        _RUNS[cid] = run
    return _RUNS[cid]


CASE_IDS = list(H.CASE_IDS)
WHIRL_IDS = [c for c in CASE_IDS if c.split("/")[0] in WHIRL_FAMILIES]
# the cases that run once more with a renderer hand-off registered (the AOS instantiations): the ragged and tiny counts, nan_clamp,
# two random configurations per sort mode and the whirl cases
AOS_IDS = sorted(set([c for c in CASE_IDS if c.split("/")[0] in ("ragged", "dam")] + ["nan_clamp"] +
                     [f"random/{k}/{s}" for k in (0, 1) for s in H.SORTS] + WHIRL_IDS), key=CASE_IDS.index)


def describe(run):
    c = run.case
    return (f"[body_cases2d] {c.name} (n {c.n}, {c.sort}, hb {run.hb}): hits {[s.hits() for s in run.steps]}, re-clamped "
            f"{[s.reclamped() for s in run.steps]}, dropped {[s.dropped() for s in run.steps]}, edge {[s.edge for s in run.steps]}, NaN after {[int(s.nan) for s in run.steps]}")


# ---- b. the operator's own guards -------------------------------------------------------------------------------------------
GUARD_N, GUARD_SEED = 4097, 31
PLANT = (0, 1, 62, 63, 64, 127, 510, 511, 512, 513, 4094, 4095, 4096)
SMALL = (1e-40, -1e-45, -0.0, -0.0, 1e-30, 0.3, -0.7, 0.0)             # uploaded velocities that a step of delta 0 leaves alone
PICK_RES = 1024


def guard_base(fs, orc):
    """(settings, offset, tick, records): the jittered block of 4097 particles in dam_break_2d's box"""
    return PS.jittered_dam_break(fs, orc, GUARD_N, GUARD_SEED)


def copy_tick(tick, **over):
    t = type(tick).from_buffer_copy(tick)
    for k, v in over.items():
        setattr(t, k, type(getattr(t, k))(*v) if isinstance(v, tuple) else v)
    return t


def picker(pos, slots, vector, **motion):
    """a body over the bounding box of the finite positions (PICK_RES^2 pixels, identity rotation) whose field holds `vector` in the
    pixels of the particles `slots` and nothing elsewhere"""
    ok = finite_rows(pos)
    lo, hi = pos[ok].min(axis=0).astype(np.float64) - 0.01, pos[ok].max(axis=0).astype(np.float64) + 0.01
    body = B.Body(np.zeros((PICK_RES, PICK_RES, 2), dtype=f32), hi - lo, centre=(lo + hi) / 2, **motion)
    ix, iy, inside = pixels(body, pos[list(slots)])
    assert inside.all()
    body.field[iy, ix] = vector
    return body


def hit_slots(rec):
    return [int(i) for i in np.flatnonzero(rec["hit"])]


def lane_pairs(rec):
    """(pairs with both halves hit, only the first, only the second) of the lanes of k_bodies: lane t holds particles 2 t, 2 t + 1"""
    hit = rec["hit"]
    n = hit.shape[0] // 2 * 2
    a, b = hit[0:n:2], hit[1:n:2]
    return int((a & b).sum()), int((a & ~b).sum()), int((~a & b).sum())


class Guard:
    """`state(p)`: the uploaded records (p is a fresh copy of the base); `tick_over`: what the tick changes; `bodies(after, size)`:
    the bodies, from the state a body-less step leaves; `check(after, want, words, recs)`: asserts that the guard meets what it
    names and returns a line to print.  reference(): (bodies, want, words, recs) on a given `after`."""

    def __init__(self, name, bodies, check, state=None, **tick_over):
        self.name, self.bodies, self.check, self.state, self.tick_over = name, bodies, check, state, tick_over

    def upload(self, base):
        p = base.copy()
        return self.state(p) if self.state else p

    def tick(self, tick):
        return copy_tick(tick, **self.tick_over)

    def reference(self, after, size, tick):
        bodies = self.bodies(after, size)
        want, words, recs = L.apply_bodies(after, bodies, size, tick.damping_factor)
        return bodies, want, words, recs


def _small_velocities(p):
    pool = np.array(SMALL, dtype=f32)
    p["velocity"] = pool[np.random.default_rng(3).integers(0, pool.size, size=p["velocity"].shape)]
    return p


def bbox_centre(pos):
    """the centre of a picker over these positions"""
    ok = finite_rows(pos)
    return (pos[ok].min(axis=0).astype(np.float64) + pos[ok].max(axis=0).astype(np.float64)) / 2


def nearest(pos, point, avoid=()):
    """the finite particle nearest to `point` that is not one of `avoid`"""
    d = ((pos.astype(np.float64) - np.asarray(point, dtype=np.float64)) ** 2).sum(axis=1)
    d[~finite_rows(pos)] = np.inf
    d[list(avoid)] = np.inf
    return int(np.argmin(d))


def makers_and_target(after, size, apply, pick, vectors, spin_up, spin_down, slide, target, offset):
    """The four bodies of the entry-velocity guard, the same in 2D and 3D.  With w = -3e38 about z and s the pushed position from
    the centre, us.x = u.x + 3e38 s.y and us.y = u.y - 3e38 s.x.
      spin_up    u = (3e38, -3e38): at s = (-0.5, 0.6) us.x overflows to +inf and us.y stays finite, so v.x = inf - inf is a NaN and the
                 other components are +inf.  It hits that particle (`up`) and every fourth particle of PLANT.
      spin_down  u = (-3e38, 3e38): at s = (0.5, -0.6) the same with -inf.  It hits `down` and another quarter of PLANT.
      slide      no spin, u.x = 3.38e38, push along +x: v.x = 0.9 u.x, finite and above 3e38.  It hits every other particle of PLANT.
      target     an ordinary motion; it hits all of PLANT and `up` and `down` where the makers left them.
    Elsewhere in the block both components of us overflow and the makers leave NaN in every component."""
    pos = after["position"]
    c = bbox_centre(pos)
    up = nearest(pos, c + offset, PLANT)
    with np.errstate(all="ignore"):
        a = pick(pos, PLANT[0::4] + (up,), vectors[0], **spin_up)
        met = apply(after, a, size, 0.1)[0]                           # (the positions a body leaves do not depend on the damping)
        down = nearest(met["position"], bbox_centre(met["position"]) - offset, PLANT + (up,))
        b = pick(met["position"], PLANT[2::4] + (down,), vectors[0], **spin_down)
        met = apply(met, b, size, 0.1)[0]
        s_ = pick(met["position"], PLANT[1::2], vectors[1], **slide)
        met = apply(met, s_, size, 0.1)[0]
    return [a, b, s_, pick(met["position"], PLANT + (up, down), vectors[2], **target)]


def _makers_and_target(after, size):
    return makers_and_target(after, size, B.apply_body, picker, [(6e-4, 8e-4), (1e-3, 0.0), (-3e-4, 4e-4)],
                             dict(velocity=(3e38, -3e38), angular_velocity=-3e38), dict(velocity=(-3e38, 3e38), angular_velocity=-3e38),
                             dict(velocity=(3.38e38, -3e38)), dict(velocity=(0.5, 0.25), angular_velocity=1.0), np.array([-0.5, 0.6]))


def _check_entry(after, want, words, recs):
    """2D and 3D: the pickers hit what they aim at and nothing else, every hit is dropped, none re-clamped, and the entry
    velocities of every kind occur"""
    extra = [i for i in hit_slots(recs[3]) if i not in PLANT]
    assert len(extra) == 2 and sorted(hit_slots(recs[3])) == sorted(PLANT + tuple(extra)), "the target hits PLANT and the two particles up and down"
    up, down = [e for e in extra if recs[0]["hit"][e]], [e for e in extra if recs[1]["hit"][e]]
    assert hit_slots(recs[0]) == sorted(PLANT[0::4] + tuple(up)) and hit_slots(recs[1]) == sorted(PLANT[2::4] + tuple(down))
    assert len(up) == 1 and len(down) == 1 and hit_slots(recs[2]) == list(PLANT[1::2])
    assert recs[0]["hit"][-1] and recs[3]["hit"][-1], "the last particle of the odd count"
    if after["position"].shape[1] == 2:                                # lanes of two particles
        assert lane_pairs(recs[0])[0] == lane_pairs(recs[1])[0] == lane_pairs(recs[2])[0] == 0, "the makers hit one half of a pair"
        both, first, second = lane_pairs(recs[3])
        assert both >= 5 and first >= 1 and second >= 1
    for w, r in zip(words, recs):
        assert w[-2] == w[-1] == int(r["hit"].sum()) and not r["clamped"].any(), "every hit dropped, none re-clamped"
    v0 = np.concatenate([r["v0"] for r in recs[:3]])
    kinds0 = {"denormal": int(((v0 != 0) & (np.abs(v0) < np.finfo(f32).tiny)).sum()), "-0.0": int(((v0 == 0) & np.signbit(v0)).sum()),
              "zero": int((v0 == 0).sum())}
    v0 = recs[3]["v0"]
    one = np.isnan(v0).sum(axis=1) == 1
    kinds1 = {"NaN in every component": int(np.isnan(v0).all(axis=1).sum()),
              "NaN in one, +inf in the others": int((one & ((v0 == np.inf) | np.isnan(v0)).all(axis=1)).sum()),
              "NaN in one, -inf in the others": int((one & ((v0 == -np.inf) | np.isnan(v0)).all(axis=1)).sum()),
              "finite, 3e38 or more": int((np.isfinite(v0) & (np.abs(v0) >= f32(3e38))).any(axis=1).sum())}
    assert kinds0["denormal"] > 0 and kinds0["-0.0"] > 0 and kinds0["zero"] > kinds0["-0.0"], kinds0
    assert min(kinds1.values()) > 0 and kinds1["finite, 3e38 or more"] == len(PLANT[1::2]), kinds1
    return f"makers' entry {kinds0}, target's entry {kinds1}"


def _positions(p):
    kinds = [(np.nan, None), (None, np.nan), (np.inf, None), (None, -np.inf), (-np.inf, np.inf)]
    for k, slot in enumerate(PLANT):
        x, y = kinds[k % len(kinds)]
        if x is not None:
            p["position"][slot, 0] = x
        if y is not None:
            p["position"][slot, 1] = y
    p["predicted_position"] = p["position"]
    return p


def _cover(size, field, **motion):
    return B.Body(np.asarray(field, dtype=f32), (2.0 * size[0], 2.0 * size[1]), **motion)


def _one(vector):
    return np.array(vector, dtype=f32).reshape(1, 1, 2)


def _centred(after, slot=2048):
    return after["position"][slot]


def _check_positions(after, want, words, recs):
    nan = np.isnan(after["position"]).any(axis=1)
    assert nan.sum() >= 4 and np.isfinite(after["position"][~nan]).all(), "the step leaves a NaN position and clamps an infinite one"
    expect("one", "none", "none", 0, MID)(after, want, words, recs)    # the particle exactly at the centre of the first body
    assert words[1][-2] == int((~nan).sum()) and not recs[1]["hit"][nan].any(), "NaN: outside; every finite particle: inside"
    assert words[1][-1] == 0 and 0 < int(recs[1]["clamped"].sum()) < words[1][-2], "the cover: no drop, some re-clamps"
    assert want["position"][nan].tobytes() == after["position"][nan].tobytes() and want["velocity"][nan].tobytes() == after["velocity"][nan].tobytes()
    return f"NaN positions {int(nan.sum())}, hits {[w[-2] for w in words]}, re-clamped {[int(r['clamped'].sum()) for r in recs]}"


def _count(kind, got, of, what):
    if kind == "all":
        assert got == of, f"{what}: {got}, expected all {of}"
    elif kind == "none":
        assert got == 0, f"{what}: {got}, expected none"
    elif kind == "one":
        assert got == 1, f"{what}: {got}, expected one"
    else:
        assert kind == "some" and 0 < got < of, f"{what}: {got}, expected some of {of}"


def expect(hits, dropped, reclamped, body=0, slot=None):
    """A check of one body of a guard, 2D or 3D: `hits` of the particles, `dropped` and `reclamped` of the hits, each 'all', 'none',
    'one' or 'some' (more than none, fewer than all); with `slot`, that particle is hit."""
    def check(after, want, words, recs):
        h, d, c = words[body][-2], words[body][-1], int(recs[body]["clamped"].sum())
        assert h == int(recs[body]["hit"].sum())
        _count(hits, h, after.shape[0], "hits")
        _count(dropped, d, h, "dropped")
        _count(reclamped, c, h, "re-clamped")
        assert slot is None or recs[body]["hit"][slot], f"particle {slot} is not hit"
        return f"hits {h}, dropped {d}, re-clamped {c}"
    return check


MID = 2048


def _no_hit(after, want, words, recs):
    assert all(x == 0 for w in words for x in w) and want.tobytes() == after.tobytes()
    return "no hit"


def _check_zero_rot(after, want, words, recs):
    line = expect("all", "none", "none")(after, want, words, recs)
    assert want["position"].tobytes() == after["position"].tobytes(), "q = 0 and f = 0: hit, not moved"
    assert want["velocity"].tobytes() != after["velocity"].tobytes()
    return line


FOUR = np.array([[[0.01, 0.0], [0.0, 0.02], [-0.03, 0.0], [0.0, -0.04]]], dtype=f32)       # 4 x 1, four distinct vectors


def denormal_extent_body(after):
    return B.Body(FOUR, (1e-40, 1.0), centre=_centred(after))


def _check_denormal_extent(after, want, words, recs):
    """(0 + hb) / extent = 0.5 from two denormals: pixel 2; with the operands flushed, 0 / 0 is a NaN and the pixel is 0"""
    body = denormal_extent_body(after)
    ix = pixels(body, after["position"][2048])[0][0]
    with np.errstate(all="ignore"):
        flushed = (flush(body.extent * f32(0.5))[0] / flush(body.extent)[0]) * f32(4)
    other = int(min(CR.u32_sat(flushed), 3))
    expect("one", "none", "none", 0, MID)(after, want, words, recs)
    assert ix == 2 and other != 2, (ix, other)
    moved = want["position"][2048] - after["position"][2048]
    assert moved[0] < 0 and moved[1] == 0, "the vector of pixel 2"
    return f"pixel {ix}, a flushed quotient gives pixel {other}"


def _eight(after, size):
    """eight bodies, each centred where the one before left the particle: up through the ceiling, down through the floor, ..."""
    out, rec = [], after
    with np.errstate(all="ignore"):
        for k in range(8):
            body = B.Body(_one((0.0, (-2.0 if k % 2 == 0 else 2.0) * size[1])), (0.02, 0.02), centre=rec["position"][4096],
                          velocity=(0.1 * k, -0.2), angular_velocity=0.5 * k)
            rec = B.apply_body(rec, body, size, 0.1)[0]               # (positions: whatever the damping)
            out.append(body)
    return out


def _check_eight(after, want, words, recs):
    for k in range(8):                                                 # the last particle: eight hits, eight re-clamps, no drop
        expect("one", "none", "all", k, after.shape[0] - 1)(after, want, words, recs)
    return f"hits {[w[-2] for w in words]}"


def _through_floor(after, size):
    return [_cover(size, _one((0.0, 2.0 * size[1])), velocity=(0.3, -0.2), angular_velocity=0.5)]


def _guards():
    c = lambda f: (lambda after, size: [f(after, size)])               # noqa: E731
    cover = lambda field, **m: c(lambda after, size: _cover(size, field, **m))      # noqa: E731
    at = lambda field, extent, **m: c(lambda after, size: B.Body(field, extent, centre=_centred(after), **m))      # noqa: E731
    wide = B.random_field((6, 5), 9, fill=1.0, mag=0.05)
    out = [
        Guard("entry_velocities", _makers_and_target, _check_entry, state=_small_velocities, delta=0.0, gravity=(-1.0, -9.81)),
        Guard("positions", lambda after, size: [B.Body(_one((0.01, 0.02)), (1e-4, 1e-4), centre=_centred(after)), _cover(size, wide)],
              _check_positions, state=_positions),
        Guard("rot/zero", at(wide, (1.0, 1.0), rot=(0.0, 0.0, 0.0, 0.0), velocity=(0.2, 0.1), angular_velocity=1.0), _check_zero_rot),
        Guard("rot/tenth", at(wide, (0.1, 0.1), rot=(0.1, 0.0, 0.0, 0.1)), expect("some", "none", "none")),
        Guard("rot/1e38", at(wide, (1.0, 1.0), rot=(1e38, 1e38, -1e38, 1e38)), expect("one", "all", "all", 0, MID)),
        Guard("rot/reflection", at(wide, (2.0, 1.5), rot=(1.0, 0.0, 0.0, -1.0), angular_velocity=1.0), expect("some", "none", "none")),
        Guard("extent/2^-149", at(wide, (2.0 ** -149, 1.0)), expect("one", "none", "none", 0, MID)),
        Guard("extent/1e-40", lambda after, size: [denormal_extent_body(after)], _check_denormal_extent),
        Guard("extent/1e30", at(wide, (1e30, 1e30)), expect("all", "none", "none")),
        Guard("extent/3e38", at(wide, (3e38, 3e38)), expect("all", "none", "none")),
        Guard("field/3e38", cover(_one((3e38, 1e30))), expect("all", "none", "all")),
        Guard("field/1e30", cover(_one((-1e30, 1e30)), velocity=(0.5, 0.5)), expect("all", "some", "all")),
        Guard("field/-0", cover(_one((-0.0, 0.0))), _no_hit),
        Guard("field/half_underflow", cover(_one((1e-40, 1e-19))), expect("all", "none", "none")),
        Guard("field/underflow", cover(_one((1e-30, 1e-30))), _no_hit),
        Guard("motion/3e38", cover(wide, velocity=(3e38, -3e38), angular_velocity=-3e38), expect("all", "all", "none")),
        Guard("eight_on_one", _eight, _check_eight),
    ]
    out += [Guard(f"damping/{d}", _through_floor, expect("all", "none", "all"), damping_factor=d) for d in (0.0, 1.0, 1.5, -0.5)]
    return out


GUARDS = {g.name: g for g in _guards()}
GUARD_IDS = list(GUARDS)
MODE_GUARD = "entry_velocities"                                        # the guard that also runs in the other two math modes

# ---- c. the loads over more than 64 workgroups ------------------------------------------------------------------------------
LOADS_WORKGROUP = 512                                                  # particles per workgroup of k_bodies_loads: 256 lanes, two each
LOADS_SHARDS = 64
MANY_WORKGROUPS = (65 * 512 + 1, 129 * 512 + 1)


def many_state(fs, orc, n):
    return PS.jittered_dam_break(fs, orc, n, n % 1000)


def many_bodies(size):
    return [_cover(size, B.random_field((9, 7), 4, fill=1.0, mag=0.08), velocity=(0.3, -0.2), angular_velocity=0.25)]
