"""The hard inputs of the plain 2D step (tests/test_parity_gpu.py, tests/test_prologue_edges_gpu.py) with the opt-in surface-tension
pass on: the cases, and the coefficient and threshold of each, chosen from the checker alone, on the CPU.  One
registry for tests/test_surface_tension_hard_inputs_gpu.py (the engine against the checker) and for the CPU companion in
tests/test_surface_tension.py (the checker alone: the cases test what they say).  No GPU.

The checker of a case is tests/st_ref.STChecker.step.  The states are those of the plain tests (tests/parity_states.py,
tests/prologue_scenes.py, tests/dense_scene.py).  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from tests import parity_states as PS
from tests import prologue_scenes as S
from tests import st_choice
from tests.dense_scene import dense_scene

f32 = np.float32
FLOAT_FIELDS = ("position", "predicted_position", "velocity", "density")
SORTS = ("bitonic", "counting")
CONTRACT_RHO = 1e-5                # density contract of FS_MATH_TOLERANCE (relative)
TOL_GAP = 1e-3                     # the threshold of a tolerance case keeps this relative distance from every |n|


def norm2(n):
    """the statement's |n| in f32: sqrt(nx * nx + ny * ny), no contraction"""
    n = np.asarray(n, dtype=f32)
    with np.errstate(all="ignore"):
        return np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1])


def copy_tick(tick, **over):
    t = type(tick).from_buffer_copy(tick)
    for k, v in over.items():
        setattr(t, k, v)
    return t


def density_state(chk, tick, stable):
    """the calls of a step up to its density pass: the state the surface-tension pass reads"""
    chk.begin_tick(tick); chk.predict(); chk.spatial_lookup()
    if stable:
        chk.sort_stable()
    else:
        chk.sort()
    chk.cell_starts(); chk.density()


def checker_step(chk, tick, stable):
    """STChecker.step(tick, stable) call for call (stc_step of tests/st_checker.cpp), keeping the pass's n and L: returns the
    (N, 3) f32 {n.x, n.y, L} of the step; chk.st holds its forces"""
    density_state(chk, tick, stable)
    st, nl = chk.surface_tension_pass()
    chk.move_st(st)
    chk.st = st
    return nl


class Step:
    """one checker step of a case: records, start_indices and forces after it, {n.x, n.y, L} and |n| of its pass, and the
    densities the pass read (the records' own: the move pass does not change them)"""

    def __init__(self, rec, start, st, nl):
        self.rec, self.start, self.st, self.nl3, self.nl = rec, start, st, nl, norm2(nl)
        for a in (self.rec, self.start, self.st, self.nl3, self.nl):
            a.setflags(write=False)

    def above(self, tau):
        with np.errstate(invalid="ignore"):
            return (self.nl > f32(tau)) & (self.nl > f32(0))


class Case:
    """One state and its settings.  `tick` carries the chosen sigma and tau (the engine reads them from the tick settings);
    `figures`: what the choice measured on the checker."""

    def __init__(self, name, st, off, tick, start, steps, quirks=True, sort="bitonic", field=None, start_indices=None):
        self.name, self.st, self.off, self.start, self.steps = name, st, (float(off[0]), float(off[1])), start, steps
        self.tick = copy_tick(tick)
        self.quirks, self.sort, self.field, self.start_indices = quirks, sort, field, start_indices
        self.sigma = self.tau = None
        self.figures = {}
        self._run = None
        self.h = float(st.smoothing_radius)

    @property
    def stable(self):
        return self.sort == "counting"

    def set_st(self, sigma=None, tau=None):
        if sigma is not None:
            self.sigma = float(sigma)
        if tau is not None:
            self.tau = float(tau)
        self.tick = copy_tick(self.tick, surface_tension_coefficient=self.sigma, surface_tension_treshold=self.tau)
        self.figures.update(sigma=self.sigma, tau=self.tau)
        self._run = None
        return self

    def checker(self):
        from tests.st_ref import STChecker
        chk = STChecker(self.st, self.off, ref_quirks=self.quirks)
        chk.set_particles(self.start)
        if self.start_indices is not None:
            chk.start_indices_view()[:] = self.start_indices
        if self.field is not None:
            chk.texture_view()[:] = self.field
        return chk

    def run(self):
        """the whole case on the checker: a list of Step; computed once.  Figures: the branch counts over all steps."""
        if self._run is None:
            chk = self.checker()
            out = []
            with np.errstate(all="ignore"):
                for _ in range(self.steps):
                    nl = checker_step(chk, self.tick, self.stable)
                    out.append(Step(chk.particles(), chk.start_indices(), chk.st.copy(), nl))
            chk.close()
            self.figures.update(
                above=[int(s.above(self.tau).sum()) for s in out], below=[int((~s.above(self.tau)).sum()) for s in out],
                nan_n=[int(np.isnan(s.nl).sum()) for s in out], zero_n=[int((s.nl == 0).sum()) for s in out])
            self._run = out
        return self._run


# ---- sigma and tau, from the checker alone ----------------------------------------------------------------------------------
def choose_surface_tension(case):
    """st_choice.choose_surface_tension on the 2D checker: the step's own acceleration is the velocity change of the plain move
    pass over dt; the force and the |n| are those of the pass on the first step's density state, with (sigma, 0)."""
    dt = float(case.tick.delta)

    def own():
        chk = case.checker()
        density_state(chk, case.tick, case.stable)
        before = chk.particles()["velocity"].astype(np.float64)
        chk.move_st(None)
        after = chk.particles()["velocity"].astype(np.float64)
        chk.close()
        return np.linalg.norm(after - before, axis=1) / dt

    def tension(sigma):
        chk = case.checker()
        density_state(chk, copy_tick(case.tick, surface_tension_coefficient=sigma, surface_tension_treshold=0.0), case.stable)
        st, nl = chk.surface_tension_pass()
        rho = chk.particles()["density"].astype(np.float64)
        chk.close()
        return np.linalg.norm(st.astype(np.float64), axis=1) / rho, norm2(nl)

    st_choice.choose_surface_tension(case, own, tension, dt)
    case.set_st()
    run = case.run()
    if not (sum(case.figures["above"]) and sum(case.figures["below"])):
        # |n| of the first step alone leaves a branch empty over the case's steps (a handful of particles with equal |n|): take
        # the gap of the |n| of every step instead, from the run with tau = 0
        case.set_st(tau=0.0)
        pooled = np.concatenate([s.nl for s in case.run()])
        case.set_st(tau=st_choice.gap_threshold(np.unique(pooled)))
        case.figures["pooled"] = True
    return case


_CASES = {}


def _cached(key, build):
    if key not in _CASES:
        _CASES[key] = build()
    return _CASES[key]


# ---- a. operand guards ------------------------------------------------------------------------------------------------------
OWN_GUARDS = ["tiny_offsets_at_rest", "nan_clamp", "coincident", "mass_tiny", "nan_next_to_everyone", "isolated/tau0", "isolated/tau-1", "tau_exact",
              "sigma-35", "sigma_inf", "tau_nan"]
GUARDS = PS.GUARD_CASES + OWN_GUARDS
NAN_CELL = (1, S.CS.BIG_ROW)       # where a NaN x takes a particle: u32sat(floor(NaN)) + 1 = column 1, its row unchanged
ISOLATED = {10: (3.0, -2.0), 500: (4.0, -1.0), 2000: (5.0, 0.0), 4000: (3.5, 1.5)}       # source index -> position, far from all
DAM_SEED = 12                      # the jittered 4096 dam break of the cases that bring no state of their own


def dam_break(fs, orc, n=4096, seed=DAM_SEED):
    return PS.jittered_dam_break(fs, orc, n, seed)


def _mass_tiny(fs, orc):
    """mass = 0.05 / (N W(0)), W(0) = 4 / (pi h^2): no arrangement of the N particles gives a raw density above 0.05, so rho is at
    the 0.1 floor everywhere in every step, and m / rho is small but finite"""
    st, off, tick, p = dam_break(fs, orc)
    top = p.shape[0] * 4.0 / (np.pi * float(st.smoothing_radius) ** 2)
    return st, off, copy_tick(tick, mass=float(f32(0.05 / top))), p


def _nan_next_to_everyone():
    """256 particles in the one cell a NaN coordinate leads to (prologue_scenes.one_cell at NAN_CELL), one of them with a NaN
    velocity component: its predicted x is a NaN in step 1 and it keeps the cell, so every particle meets a NaN r2 — density and
    tension admit the candidate (`!(r2 > h2)`), every density falls to the floor and every |n| is a NaN: no force in step 1 by the
    statement, forces from step 2 on (the step zeroes a NaN velocity, the position never was a NaN)"""
    st, tick, p = S.one_cell(cell=NAN_CELL)
    p = p.copy()
    p["velocity"][5] = (np.nan, 0.0)
    return st, (0.0, 0.0), tick, p


def _tiny_offsets_at_rest(fs, orc):
    """What tiny_offsets of the plain suite sets out to have: there the offsets are added to a coordinate of a few units, vanish in
    its rounding (seven coincident particles at the origin), and the jittered velocities would spread the predicted positions by
    millimetres anyway.  Here seven particles sit at the origin and at offsets of 2^-149 .. 1e-7 from it, where such offsets are
    representable, at rest, so that the predict step of step 1 keeps them: r2 underflows to 0 and to denormals between
    candidates that do not coincide."""
    st, off, tick, p = PS.jittered_dam_break(fs, orc, 4096, PS.GUARD_SEED)
    p["position"][100] = 0
    for k, d in enumerate([1e-45, 1e-40, 1e-30, 1e-19, 3e-13, 1e-7]):
        p["position"][101 + k] = f32(d) * np.array([1, 0 if k % 2 else 1], f32)
    p["velocity"][100:107] = 0
    p["predicted_position"] = p["position"]
    return st, off, tick, p


def _isolated(fs, orc):
    st, off, tick, p = dam_break(fs, orc)
    for i, xy in ISOLATED.items():
        p["position"][i] = xy
        p["velocity"][i] = 0
    p["predicted_position"] = p["position"]
    return st, off, tick, p


def guard_case(fs, orc, name):
    def build():
        steps = 3
        if name in PS.GUARD_CASES:
            st, off, tick, p = PS.jittered_dam_break(fs, orc, 4096, PS.GUARD_SEED, **PS.guard_overrides(name))
            p = PS.guard_state(orc, st, p, name)
        elif name == "tiny_offsets_at_rest":
            st, off, tick, p = _tiny_offsets_at_rest(fs, orc)
        elif name == "nan_clamp":
            st, off, tick = PS.pair_settings(fs, 4096)
            p = PS.nan_clamp_state(PS.jitter(PS.lattice(orc, st, off), PS.NAN_CLAMP["seed"], PS.NAN_CLAMP["vel"]))
            steps = 4
        elif name == "coincident":
            st, off, tick, p = PS.jittered_dam_break(fs, orc, 4096, PS.COINCIDENT["seed"])
            p = PS.coincident_state(p)
        elif name == "mass_tiny":
            st, off, tick, p = _mass_tiny(fs, orc)
        elif name == "nan_next_to_everyone":
            st, off, tick, p = _nan_next_to_everyone()
        elif name.startswith("isolated/"):
            st, off, tick, p = _isolated(fs, orc)
        else:
            st, off, tick, p = dam_break(fs, orc)
            if name == "tau_exact":
                steps = 1
        case = choose_surface_tension(Case(f"guard/{name}", st, off, tick, p, steps))
        if name.startswith("isolated/"):
            case.set_st(tau={"tau0": 0.0, "tau-1": -1.0}[name.split("/")[1]])
        elif name == "tau_exact":
            _tau_exact(case)
        elif name == "sigma-35":
            case.set_st(sigma=-35.0)
        elif name == "sigma_inf":
            case.set_st(sigma=np.inf)
        elif name == "tau_nan":
            case.set_st(tau=np.nan)
        return case
    return _cached(("guard", name), build)


def _tau_exact(case):
    """tau = the f32 |n| of one particle of step 1: the median of the finite, non-zero values that no other particle shares.
    figures: `exact` = its sorted slot, `next` = the slot of the next larger |n|"""
    case.set_st(tau=0.0)
    nl = case.run()[0].nl
    vals, first, counts = np.unique(nl, return_index=True, return_counts=True)
    ok = np.isfinite(vals) & (vals > 0) & (counts == 1)
    ok[-1] = False                                                 # a larger value must follow
    k = np.nonzero(ok)[0]
    k = int(k[k.shape[0] // 2])
    case.set_st(tau=float(vals[k]))
    case.figures.update(exact=int(first[k]), next=int(first[k + 1]))


# ---- b. smoothing radii -----------------------------------------------------------------------------------------------------
RADIUS_SIDE = 45                   # 45^2 = 2025 particles


def radius_case(fs, orc, h):
    """a jittered lattice of 2025 particles at spacing 0.5 h in a box of 2 x 1.5 block sides (plus 4 h), velocities up to 5 h / s
    per component, 3 steps: Cg = 24/(pi h^8) runs from 1.5e0 (h = 1) to 2e11 (h = 0.05)"""
    def build():
        n, sp = RADIUS_SIDE ** 2, 0.5 * h
        side = RADIUS_SIDE * sp
        st = fs.SimulationSettings(n, sp, h, (2.0 * side + 4 * h, 1.5 * side + 4 * h))
        tick = fs.default_tick_settings(gravity=(0.0, 9.81))
        p = PS.jitter(PS.lattice(orc, st, (0.0, 0.0)), int(round(1000 * h)), vel=5.0 * h, jitter=0.3 * sp)
        return choose_surface_tension(Case(f"radius/{h}", st, (0.0, 0.0), tick, p, 3))
    return _cached(("radius", h), build)


# ---- c. random configurations -----------------------------------------------------------------------------------------------
def random_case(fs, orc, k, sort):
    """configuration k of test_random_configurations in the given sort mode (each mode has its own draw of the state, as there),
    ref_quirks on for even k and off for odd k, 4 steps"""
    def build():
        st, off, tick, runs = PS.random_configuration(fs, orc, k)
        _, p, field = runs[SORTS.index(sort)]
        return choose_surface_tension(Case(f"random/{k}/{sort}", st, off, tick, p, 4, quirks=k % 2 == 0, sort=sort, field=field))
    return _cached(("random", k, sort), build)


# ---- d. grid edges ----------------------------------------------------------------------------------------------------------
SMALL_DAMS = [2, 3, 5]
EDGE_CASES = [f"corners/{q}/{s}" for q in ("quirks", "noquirks") for s in SORTS] + \
    [f"ragged/{n}/{s}" for n in S.RAGGED_N for s in SORTS] + [f"dam/{n}" for n in SMALL_DAMS]


def edge_case(fs, orc, name):
    def build():
        parts = name.split("/")
        if parts[0] == "corners":
            st, tick, p = S.corners()
            return choose_surface_tension(Case(f"edge/{name}", st, (0.0, 0.0), tick, p.copy(), 3, quirks=parts[1] == "quirks", sort=parts[2]))
        if parts[0] == "ragged":
            st, tick, p = S.ragged(int(parts[1]))
            return choose_surface_tension(Case(f"edge/{name}", st, (0.0, 0.0), tick, p.copy(), 3, sort=parts[2]))
        n = int(parts[1])
        st, off, tick, p = PS.jittered_dam_break(fs, orc, n, n, size=PS.RAGGED_BOX)
        return choose_surface_tension(Case(f"edge/{name}", st, off, tick, p, 4))
    return _cached(("edge", name), build)


# ---- e. mouse and field -----------------------------------------------------------------------------------------------------
def mouse_field_case(fs, orc):
    def build():
        over = dict(PS.MOUSE_FIELD)
        seed = over.pop("seed")
        st, off, tick, p = PS.jittered_dam_break(fs, orc, 4096, seed, **over)
        return choose_surface_tension(Case("mouse_field", st, off, tick, p, 4, field=PS.mouse_field()))
    return _cached(("mouse_field",), build)


# ---- f. host case -----------------------------------------------------------------------------------------------------------
def host_case(fs, orc, sort="bitonic", quirks=True):
    """the jittered 4096 dam break, 6 steps"""
    def build():
        st, off, tick, p = dam_break(fs, orc)
        return choose_surface_tension(Case(f"host/dam4096/{sort}/{'quirks' if quirks else 'noquirks'}", st, off, tick, p, 6,
                                           quirks=quirks, sort=sort))
    return _cached(("host", sort, quirks), build)


def switch_cases(fs, orc):
    """the two scenes of the A/B-switch children, 3 steps each: the jittered 5000-particle dam break and dense_scene"""
    def build():
        st, off, tick, p = dam_break(fs, orc, 5000, 5000)
        a = choose_surface_tension(Case("switch/dam5000", st, off, tick, p, 3))
        st, tick, p = dense_scene(fs)
        b = choose_surface_tension(Case("switch/dense", st, (0.0, 0.0), tick, p, 3))
        return a, b
    return _cached(("switch",), build)


# ---- the other math modes ---------------------------------------------------------------------------------------------------
def pairs_within(q, h):
    """(i, j) of every ordered pair, i == j included, whose cells (side h) touch — a superset of the pairs within h; plain numpy"""
    n = q.shape[0]
    c = np.floor(q / h).astype(np.int64)
    c -= c.min(0)
    width = int(c[:, 0].max()) + 3
    key = (c[:, 1] + 1) * width + c[:, 0] + 1
    order = np.argsort(key, kind="stable")
    ks = key[order]
    out_i, out_j = [], []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            nk = key + dy * width + dx
            lo, hi = np.searchsorted(ks, nk, "left"), np.searchsorted(ks, nk, "right")
            cnt = hi - lo
            i = np.repeat(np.arange(n), cnt)
            within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            out_i.append(i)
            out_j.append(order[np.repeat(lo, cnt) + within])
    return np.concatenate(out_i), np.concatenate(out_j)


def tolerance_force_bound(case, rec, cg):
    """Per particle and component, how far a FS_MATH_TOLERANCE step's surface-tension force may lie from the checker's `st`, from
    the mode's stated density contract alone (features3d.tolerance_force_bound with the 2D kernel).  The pass is the IEEE one in
    both; its only perturbed input is rho_j (1e-5 relative, so w_j = m / rho_j as well), and the two f32 sums round differently
    once their terms differ.  With tn_j = w_j Cg d^2 o and tl_j = w_j (Cl d)(3 r^2 - h^2), Cl = 2 Cg, the terms of n and L
    evaluated here in float64 on the checker's state (`rec`: the records after the step, whose predicted positions and densities
    are the pass's inputs; `cg`: the uniform's f32 poly6_kernel_derivative) and K the in-radius count,
        eps = 1e-5 + 2 (K + 8) 2^-24,   |dn| <= eps sum|tn_j|,   |dL| <= eps sum|tl_j|,
    and for st = (-sigma L / |n|) n, whose direction moves by at most 2 |dn| / |n|,
        |dst| <= sigma (|dL| + 2 |L| |dn| / |n|) + 4 * 2^-24 |st|     (the last term: the final quotient and products).
    Returns (bound [N], K [N], |n| [N] in float64, |dn| [N])."""
    h2 = float(f32(case.h) * f32(case.h))
    cg = float(f32(cg))
    q = rec["predicted_position"].astype(np.float64)
    w = float(f32(case.tick.mass)) / rec["density"].astype(np.float64)
    n_ = rec.shape[0]
    i, j = pairs_within(q, float(f32(case.h)))
    o = q[j] - q[i]
    r2 = (o * o).sum(1)
    near = r2 <= h2
    i, j, o, r2 = i[near], j[near], o[near], r2[near]
    d = h2 - r2
    tn = (w[j] * (cg * d * d))[:, None] * o
    tl = w[j] * ((2.0 * cg) * d * (3.0 * r2 - h2))
    K = np.bincount(i, minlength=n_)
    nsum = np.stack([np.bincount(i, tn[:, a], n_) for a in (0, 1)], axis=1)
    nabs = np.stack([np.bincount(i, np.abs(tn[:, a]), n_) for a in (0, 1)], axis=1)
    L, labs = np.bincount(i, tl, n_), np.bincount(i, np.abs(tl), n_)
    u = 2.0 ** -24
    eps = CONTRACT_RHO + 2 * (K + 8) * u
    nl = np.linalg.norm(nsum, axis=1)
    dn = eps * np.linalg.norm(nabs, axis=1)
    sigma = abs(case.sigma)
    with np.errstate(all="ignore"):
        bound = np.where(nl > 0, sigma * (eps * labs + 2 * np.abs(L) * dn / nl) + 4 * u * sigma * np.abs(L), 0.0)
    return bound, K, nl, dn


def choose_tolerance_threshold(case, cg):
    """tau of a tolerance case: the middle of a relative gap of the |n| of the case's one step that (a) is at least 2 TOL_GAP wide,
    so that tau keeps TOL_GAP (a hundred times the density contract) from every |n|, and (b) no particle can cross under the
    density contract: | |n| - tau | > |dn| of tolerance_force_bound for every particle.  Of the gaps that meet both, the one that
    splits the particles most evenly (16384 values lie closer than (a) asks for around their median: the gap is in a tail).
    figures: `tau_gap` = min | |n| / tau - 1 |, `tau_margin` = min (| |n| - tau | / |dn|)."""
    case.set_st(tau=0.0)
    step = case.run()[0]
    _, _, _, dn = tolerance_force_bound(case, step.rec, cg)
    nlf = step.nl.astype(np.float64)
    vals = np.unique(nlf[np.isfinite(nlf) & (nlf > 0)])
    ratio = vals[1:] / vals[:-1]
    wide = np.nonzero(ratio >= (1 + TOL_GAP) ** 2)[0]
    below = np.searchsorted(np.sort(nlf), vals[wide], "right")            # particles at or below the gap's lower end
    for k in wide[np.argsort(-np.minimum(below, nlf.shape[0] - below), kind="stable")]:
        tau = float(f32(np.sqrt(vals[k] * vals[k + 1])))
        margin = np.abs(nlf - tau) / np.maximum(dn, 1e-300)
        if margin.min() > 1.0:
            case.set_st(tau=tau)
            case.figures.update(tau_gap=float(np.abs(nlf[nlf > 0] / tau - 1).min()), tau_margin=float(margin.min()))
            return case
    raise AssertionError(f"{case.name}: no gap of |n| is safe under the density contract")


TOL_CASES = ["dam16384/mass1", "dam16384/mass1.25", "dense"]


def tolerance_case(fs, orc, name):
    """one step from a checker state.  dam16384: the disordered 16384 dam break of test_other_math_modes_within_contract after
    three checker steps (with the case's mass), records and start_indices; dense: dense_scene as uploaded."""
    def build():
        if name == "dense":
            st, tick, p = dense_scene(fs)
            case = Case("tol/dense", st, (0.0, 0.0), tick, p, 1)
        else:
            from tests.st_ref import STChecker
            st, off, tick, p = PS.disordered_dam_break(fs)
            tick = copy_tick(tick, mass=float(name.split("mass")[1]))
            chk = STChecker(st, off)
            chk.set_particles(p)
            for _ in range(3):
                chk.step(tick)
            case = Case(f"tol/{name}", st, off, tick, chk.particles(), 1, start_indices=chk.start_indices())
            chk.close()
        choose_surface_tension(case)
        return choose_tolerance_threshold(case, fs.build_uniform(case.st, case.tick, 1).poly6_kernel_derivative)
    return _cached(("tol", name), build)


# ---- the registry -----------------------------------------------------------------------------------------------------------
def all_cases(fs, orc):
    """(id, builder) of every case of families a. to e., in the order the GPU file runs them"""
    out = [(f"guard/{g}", lambda g=g: guard_case(fs, orc, g)) for g in GUARDS]
    out += [(f"radius/{h}", lambda h=h: radius_case(fs, orc, h)) for h in PS.RADII]
    out += [(f"random/{k}/{s}", lambda k=k, s=s: random_case(fs, orc, k, s)) for k in range(PS.RANDOM_CASES) for s in SORTS]
    out += [(f"edge/{e}", lambda e=e: edge_case(fs, orc, e)) for e in EDGE_CASES]
    out += [("mouse_field", lambda: mouse_field_case(fs, orc))]
    return out


CASE_IDS = [cid for cid, _ in all_cases(None, None)]


def case_by_id(fs, orc, cid):
    return dict(all_cases(fs, orc))[cid]()


def describe(case):
    f = case.figures
    keys = ("sigma", "tau", "n", "with_n", "own_dv", "st_dv", "above", "below", "nan_n", "zero_n", "pooled", "exact", "next",
            "tau_gap", "tau_margin")
    return f"[features2d] {case.name} ({case.sort}, quirks {int(case.quirks)}): " + \
        ", ".join(f"{k} {f[k]:.6g}" if isinstance(f[k], float) else f"{k} {f[k]}" for k in keys if k in f)
