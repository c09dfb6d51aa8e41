"""The hard inputs of the plain 3D step (tests/test_3d_paths_gpu.py) with the two opt-in passes on: the cases, and the feature
settings of each — the surface-tension coefficient and threshold, the collider field — chosen from the checker alone, on the
CPU.  One registry for tests/test_3d_features_hard_inputs_gpu.py (the engine against the checker) and for the CPU companions in
tests/test_surface_tension3d.py and tests/test_collide3d.py (the checker alone: the cases test what they say).  No GPU.

The checker of a case is C(ST3Checker.step(state)) with the result set back each step: ST3Checker with cfg = None is the plain
oracle step, C is tests/collide3d_ref.apply_collider.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import paths3d
from tests import collide3d_ref as CR
from tests import st3d_ref as R
from tests.st_choice import choose_surface_tension as _choose
from tests.track_ref import jitter_velocities

f32 = np.float32
SCENE_ST = (0.02, 0.5)             # (sigma, tau) of the path scenes: tests/test_surface_tension3d.py imports it from here
FIELD_SHAPE = (7, 5, 3)            # (W, H, D): extents that divide nothing
FIELD_SHAPES_TOL = [(7, 5, 3), (5, 3, 2), (3, 2, 1)]      # candidates of the tolerance-mode collider case, first that fits
OWN_CASES = ["mass_tiny", "positions_on_plus_b", "nan_next_to_everyone"]
GUARDS = paths3d.GUARD_CASES + OWN_CASES
TOL_SCENES = sorted(paths3d.scenes())
LONGEST_ROW = max((s for s in TOL_SCENES if s.startswith("row")), key=lambda s: int(s[3:]))
CONTRACT_POS = 1e-4                # position contract of FS_MATH_TOLERANCE, in units of h


def norm3(n):
    return np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])


class Case:
    """One state and its feature settings.  `steps`: compared steps; `field`: None or the collider; `sigma`, `tau`: None (pass
    off) or the surface-tension setting; `figures`: what the choice of the settings measured on the checker."""

    def __init__(self, name, st, off, tick, start, steps):
        self.name, self.st, self.off, self.tick, self.start, self.steps = name, st, off, tick, start, steps
        self.sigma = self.tau = self.field = None
        self.figures = {}
        self._run = None
        self.size = (st.size.x, st.size.y, st.size.z)
        self.h = float(st.smoothing_radius)

    @property
    def cfg(self):
        return None if self.sigma is None else (self.sigma, self.tau)

    def checker(self):
        chk = R.ST3Checker(self.st, self.off)
        chk.set_particles(self.start)
        return chk

    def checker_step(self, chk, want_acc=False):
        """one step of the case's checker: (records after C, records before C, pushed, re-clamped, acc)"""
        with np.errstate(all="ignore"):
            acc = chk.step(self.tick, self.cfg, want_acc=want_acc)
            pre = chk.particles()
            if self.field is None:
                return pre, pre, 0, 0, acc
            rec, pushed, reclamped = CR.apply_collider(pre, self.field, self.size, self.tick.damping_factor)
        chk.set_particles(rec)
        return rec, pre, pushed, reclamped, acc

    def run(self):
        """the whole case on the checker: a list of (records, st or None) per step, and the totals; computed once"""
        if self._run is None:
            chk = self.checker()
            out, pushed, reclamped = [], 0, 0
            for _ in range(self.steps):
                rec, _, a, b, _ = self.checker_step(chk)
                rec.setflags(write=False)
                out.append((rec, None if self.cfg is None else chk.st.copy()))
                pushed += a; reclamped += b
            chk.close()
            self.figures.update(pushed=pushed, reclamped=reclamped)
            self._run = out
        return self._run


# ---- the feature settings, from the checker alone -----------------------------------------------------------------------
def choose_surface_tension(case):
    """st_choice.choose_surface_tension on the 3D checker: the step's own acceleration is |acc / rho + g| (the checker's acc, plain
    step); the force and the |n| are those of one step with (sigma, 0)."""
    def own():
        chk = case.checker()
        acc = chk.step(case.tick, None, want_acc=True).astype(np.float64)
        rho = chk.particles()["density"].astype(np.float64)
        g = np.array([case.tick.gravity.x, case.tick.gravity.y, case.tick.gravity.z], dtype=np.float64)
        chk.close()
        return np.linalg.norm(acc / rho[:, None] + g, axis=1)

    def tension(sigma):
        chk = case.checker()
        chk.step(case.tick, (sigma, 0.0))
        nl = norm3(chk.surface_tension_pass(sigma, 0.0)[0])
        unit = np.linalg.norm(chk.st.astype(np.float64), axis=1) / chk.particles()["density"].astype(np.float64)
        chk.close()
        return unit, nl

    return _choose(case, own, tension, case.tick.delta)


def choose_collider(case, shape=FIELD_SHAPE, seed=None):
    """a random field (collide3d_ref.random_field) with components up to h; a one-voxel field is never the zero vector"""
    seed = sum(ord(c) for c in case.name) if seed is None else seed
    case.field = CR.random_field(shape, seed, fill=1.0 if tuple(shape) == (1, 1, 1) else 0.5, mag=case.h)
    case.figures.update(field=tuple(shape))
    return case


def face_distance(pre, field, size):
    """world distance of every position to the nearest voxel face of the look-up of C, per particle (inf where non-finite)"""
    D, H, W = field.shape[:3]
    out = np.full(pre.shape[0], np.inf)
    with np.errstate(all="ignore"):
        for a, wa in enumerate((W, H, D)):
            s = float(f32(size[a]))
            x = (pre["position"][:, a].astype(np.float64) + s / 2) / s * wa
            d = np.abs(x - np.round(x)) * s / wa
            d = np.where((np.round(x) <= 0) | (np.round(x) >= wa), np.inf, d)        # the box's own faces: the index is clamped
            out = np.minimum(out, np.where(np.isfinite(x), d, np.inf))
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------
_CASES = {}
FEATURES = ("st", "st+collide")


def _finish(case, features, thin=False):
    choose_surface_tension(case)
    if features == "st+collide":
        choose_collider(case, (1, 1, 1) if thin == "one" else FIELD_SHAPE)
    return case


def _mass_tiny(fs, orc):
    """mass = 0.05 / (the largest density of the state at mass 1): every raw density is below the floor, so rho is 0.1
    everywhere and m / rho is small but finite"""
    ref, st, tick, p = paths3d.pair3_state(fs, orc, 12)
    ref.close()
    chk = R.ST3Checker(st)
    chk.set_particles(p); chk.step(tick, None)
    top = float(chk.particles()["density"].max())
    chk.close()
    ref, st, tick, p = paths3d.pair3_state(fs, orc, 12, mass=float(f32(0.05 / top)))
    ref.close()
    return st, tick, p


def _positions_on_plus_b(fs, orc):
    """the side-12 lattice with 26 particles uploaded exactly at +b / -b (every face, edge and corner) and moving outwards: the
    step clamps them onto the wall again, so C sees (p + b) / size == 1 on every axis"""
    ref, st, tick, p = paths3d.pair3_state(fs, orc, 12)
    ref.close()
    b = f32(st.size.x) * f32(0.5)
    signs = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]
    for j, sg in enumerate(signs):
        s = np.array(sg, dtype=f32)
        p["position"][j] = np.where(s != 0, s * b, p["position"][j])
        p["velocity"][j] = np.where(s != 0, s * (np.abs(p["velocity"][j]) + f32(1)), p["velocity"][j])
    p["predicted_position"] = p["position"]
    return st, tick, p


def _nan_next_to_everyone(fs, orc):
    """the one-cell box of the thin grids with one NaN velocity component: in step 1 that particle's predicted x is a NaN while it
    stays in the only cell, so every particle meets a NaN r2 — density and tension admit the candidate (`!(r2 > h2)`), every
    density falls to the floor and every |n| is a NaN: no force in step 1 by the statement, forces in steps 2 and 3 (the step
    zeroes a NaN velocity, the position never was a NaN)"""
    st, tick, p = paths3d.thin_state(fs, orc, paths3d.THIN_SIZES[0])
    p["velocity"][5] = (np.nan, 0.0, 0.0)
    return st, tick, p


def guard_case(fs, orc, name, features):
    key = ("guard", name, features)
    if key not in _CASES:
        if name == "mass_tiny":
            st, tick, p = _mass_tiny(fs, orc)
        elif name == "positions_on_plus_b":
            st, tick, p = _positions_on_plus_b(fs, orc)
        elif name == "nan_next_to_everyone":
            st, tick, p = _nan_next_to_everyone(fs, orc)
        else:
            ref, st, tick, p = paths3d.pair3_state(fs, orc, 12, **paths3d.guard_overrides(name))
            ref.close()
            p = paths3d.guard_state(orc, st, p, name)
            p["predicted_position"] = p["position"]                      # as run3 uploads it
        case = _finish(Case(f"guard/{name}/{features}", st, (0.0, 0.0, 0.0), tick, p, 3), features)
        if name == "positions_on_plus_b" and case.field is not None:     # the last voxel along each axis pushes
            f = case.field
            f[-1, :, :] = np.where((f[-1, :, :] == 0).all(-1, keepdims=True), f32(0.03), f[-1, :, :])
            f[:, -1, :] = np.where((f[:, -1, :] == 0).all(-1, keepdims=True), f32(-0.02), f[:, -1, :])
            f[:, :, -1] = np.where((f[:, :, -1] == 0).all(-1, keepdims=True), f32(0.01), f[:, :, -1])
        _CASES[key] = case
    return _CASES[key]


def radius_case(fs, orc, h):
    key = ("radius", h)
    if key not in _CASES:
        ref, st, tick, p = paths3d.radius_state(fs, orc, h)
        ref.close()
        _CASES[key] = _finish(Case(f"radius/{h}", st, (0.0, 0.0, 0.0), tick, p, 3), "st")
    return _CASES[key]


RANDOM_CASES = 12


def random_case(fs, orc, k):
    key = ("random", k)
    if key not in _CASES:
        st, off, tick, mutate, desc = paths3d.random_case(fs, k)
        ref = orc.OracleSim3D(st, off)
        p = mutate(ref.particles())
        ref.close()
        case = _finish(Case(f"random/{k}", st, off, tick, p, 4), "st+collide")
        case.figures["desc"] = desc
        _CASES[key] = case
    return _CASES[key]


EDGE_CASES = ["faces/exact", "faces/inexact"] + [f"thin/{i}" for i in range(len(paths3d.THIN_SIZES))] + \
    [f"thin/{i}/one_voxel" for i in range(len(paths3d.THIN_SIZES))] + [f"wall/{a}{'+' if s > 0 else '-'}" for a, s in paths3d.WALLS]


def edge_case(fs, orc, name):
    key = ("edge", name)
    if key not in _CASES:
        parts = name.split("/")
        thin = False
        if parts[0] == "faces":
            st, tick, p = paths3d.faces_state(fs, orc, parts[1] == "exact")
            steps = 4
        elif parts[0] == "thin":
            st, tick, p = paths3d.thin_state(fs, orc, paths3d.THIN_SIZES[int(parts[1])])
            steps, thin = 3, ("one" if len(parts) == 3 else True)
        else:
            ref, st, tick, p = paths3d.wall_state(fs, orc, int(parts[1][0]), 1 if parts[1][1] == "+" else -1)
            ref.close()
            steps = 4
        _CASES[key] = _finish(Case(f"edge/{name}", st, (0.0, 0.0, 0.0), tick, p, steps), "st+collide", thin)
    return _CASES[key]


def _sensitivity(case, base):
    """the rule of test_3d_random_configurations_tolerance_mode on the case's checker: the largest change of its velocities, in
    units of the contract (2e-5 + 1e-5 |v|), when the mass moves by one ulp either way"""
    worst = 0.0
    for towards in (10.0, -10.0):
        t2 = type(case.tick).from_buffer_copy(case.tick)
        t2.mass = float(np.nextafter(f32(case.tick.mass), f32(towards)))
        chk = case.checker()
        with np.errstate(all="ignore"):
            chk.step(t2, case.cfg)
        q = chk.particles(); chk.close()
        if not np.array_equal(q["grid"], base["grid"]):
            return np.inf
        d = np.abs(q["velocity"].astype(np.float64) - base["velocity"]) / (2e-5 + 1e-5 * np.abs(base["velocity"].astype(np.float64)))
        worst = max(worst, float(np.nanmax(d)))
    return worst


def _st_dv(case):
    chk = case.checker()
    chk.step(case.tick, case.cfg)
    dv = np.linalg.norm(chk.st.astype(np.float64), axis=1) * float(case.tick.delta) / chk.particles()["density"]
    nl = norm3(chk.surface_tension_pass(*case.cfg)[0])
    chk.close()
    return float(dv.max()), nl


def tolerance_force_bound(case, rec):
    """Per particle and component, how far a FS_MATH_TOLERANCE step's surface-tension force may lie from the checker's `st`, from
    the mode's stated density contract alone.  The pass is the IEEE one in both; its only perturbed input is rho_j (1e-5 relative,
    so w_j = m / rho_j as well), and the two f32 sums round differently once their terms differ.  With tn_j, tl_j the terms of n
    and L evaluated here in float64 on the checker's state and K the in-radius count,
        eps = 1e-5 + 2 (K + 8) 2^-24,   |dn| <= eps sum|tn_j|,   |dL| <= eps sum|tl_j|,
    and for st = (-sigma L / |n|) n, whose direction moves by at most 2 |dn| / |n|,
        |dst| <= sigma (|dL| + 2 |L| |dn| / |n|) + 4 * 2^-24 |st|     (the last term: the final quotient and products).
    Returns (bound [N, 3] broadcast from [N], K [N]); rows whose checker force is zero get 0: the branch must not change (the
    CPU companion asserts that tau lies in a gap of |n| a hundred times wider than the density contract)."""
    h2 = float(f32(case.h) * f32(case.h))
    cg = 6.0 * 315.0 / (64.0 * np.pi * float(f32(case.h)) ** 9)
    q = rec["predicted_position"].astype(np.float64)
    w = float(f32(case.tick.mass)) / rec["density"].astype(np.float64)
    n_ = rec.shape[0]
    bound, count = np.zeros(n_), np.zeros(n_, dtype=np.int64)
    u = 2.0 ** -24
    for i in range(n_):
        o = q - q[i]
        r2 = (o * o).sum(1)
        near = r2 <= h2
        o, r2, wj = o[near], r2[near], w[near]
        d = h2 - r2
        tn = (wj * (cg * d * d))[:, None] * o
        tl = wj * (cg * d * (7.0 * r2 - 3.0 * h2))
        K = int(near.sum())
        eps = 1e-5 + 2 * (K + 8) * u
        nl, L = float(np.linalg.norm(tn.sum(0))), float(tl.sum())
        count[i] = K
        if nl > 0:
            dn = eps * float(np.linalg.norm(np.abs(tn).sum(0)))
            bound[i] = case.sigma * (eps * float(np.abs(tl).sum()) + 2 * abs(L) * dn / nl) + 4 * u * case.sigma * abs(L)
    return bound, count


TOL_CASES = TOL_SCENES + [LONGEST_ROW + "+collide"]


def tolerance_case(fs, orc, name):
    """a path scene with SCENE_ST, one step.  A scene whose checker moves by more than the contract under a one-ulp change of the
    mass runs with sigma halved until the checker's |st| dt / rho is below 1 m/s (figures: `lowered`).  "+collide": a field whose
    extents leave at most 1 % of the particles within the position contract of a voxel face (figures: `left_out`)."""
    key = ("tol", name)
    if key not in _CASES:
        scene = paths3d.scenes()[name.split("+")[0]]
        st, tick, p = paths3d.build_state(fs, scene)
        case = Case(f"tol/{name}", st, (0.0, 0.0, 0.0), tick, p, 1)
        case.sigma, case.tau = SCENE_ST
        chk = case.checker(); chk.step(tick, case.cfg); base = chk.particles(); chk.close()
        sens = _sensitivity(case, base)
        dv, nl = _st_dv(case)
        lowered = False
        if sens > 1.0:
            while dv >= 1.0:
                case.sigma *= 0.5
                dv, nl = _st_dv(case)
                lowered = True
        pos = np.isfinite(nl) & (nl > 0)
        case.figures.update(sigma=case.sigma, tau=case.tau, sensitivity=sens, lowered=lowered, st_dv_max=dv, n=int(nl.shape[0]),
                            with_n=int(pos.sum()), above=int((pos & (nl > f32(case.tau))).sum()),
                            below=int((pos & ~(nl > f32(case.tau))).sum()),
                            tau_gap=float(np.abs(nl[pos].astype(np.float64) / case.tau - 1).min()) if pos.any() else np.inf)
        if name.endswith("+collide"):
            for shape in FIELD_SHAPES_TOL:
                choose_collider(case, shape)
                chk = case.checker()
                _, pre, _, _, _ = case.checker_step(chk)
                chk.close()
                near = face_distance(pre, case.field, case.size) <= CONTRACT_POS * case.h
                case.figures.update(left_out=int(near.sum()))
                if near.sum() <= 0.01 * near.shape[0]:
                    break
        _CASES[key] = case
    return _CASES[key]


def host_case(fs):
    """dam_break_3d(16^3) with jittered velocities, both features, 6 steps"""
    key = ("host",)
    if key not in _CASES:
        st, off, tick = fs.dam_break_3d(16 ** 3)
        chk = R.ST3Checker(st, off)
        start = jitter_velocities(chk.particles(), 11)
        chk.close()
        case = choose_collider(choose_surface_tension(Case("host/dam16", st, off, tick, start, 6)))
        _CASES[key] = case
    return _CASES[key]


def all_cases(fs, orc):
    """(id, builder) of every case of families a. to e., in the order the GPU file runs them"""
    out = []
    for feat in FEATURES:
        out += [(f"guard/{g}/{feat}", lambda g=g, feat=feat: guard_case(fs, orc, g, feat)) for g in GUARDS]
    out += [(f"radius/{h}", lambda h=h: radius_case(fs, orc, h)) for h in paths3d.RADII]
    out += [(f"random/{k}", lambda k=k: random_case(fs, orc, k)) for k in range(RANDOM_CASES)]
    out += [(f"edge/{e}", lambda e=e: edge_case(fs, orc, e)) for e in EDGE_CASES]
    out += [(f"tol/{t}", lambda t=t: tolerance_case(fs, orc, t)) for t in TOL_CASES]
    return out


CASE_IDS = [cid for cid, _ in all_cases(None, None)]


def case_by_id(fs, orc, cid):
    return dict(all_cases(fs, orc))[cid]()


def describe(case):
    f = case.figures
    keys = ("desc", "sigma", "tau", "n", "with_n", "above", "below", "own_dv", "st_dv", "st_dv_max", "sensitivity", "lowered",
            "tau_gap", "field", "pushed", "reclamped", "left_out")
    return f"[features3d] {case.name}: " + ", ".join(f"{k} {f[k]:.6g}" if isinstance(f[k], float) else f"{k} {f[k]}" for k in keys if k in f)
