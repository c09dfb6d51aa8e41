"""The hard inputs of the plain 2D step, as ONE registry for the opt-in features that read what those inputs stress: particle
tracking (tests/test_tracking_hard_inputs_gpu.py, CPU companion in tests/test_tracking.py) and field sampling
(tests/test_sampling_hard_inputs_gpu.py, CPU companion in tests/test_sampling.py).  TEST INFRASTRUCTURE ONLY: plain numpy on the
unchanged oracle, no GPU.

The states are those of the plain tests, taken from their builders (tests/parity_states.py, tests/prologue_scenes.py,
tests/csort_scenes.py, tests/dense_scene.py): the eight operand-guard scenes, the NaN / speed-clamp / outside-the-box scene, the
coincident particles, mouse impulse with an obstacle field, the ragged dam breaks, the sixteen random configurations in both sort
modes, dense_scene, the corner clusters, the ragged counts, the staging scenes, and the counting-sort scenes that
tests/test_csort_gpu.py runs as whole steps.

A case is a name, settings, an offset, a tick, start records, a number of steps (at least 3) and optionally a field, start
indices, a quirks setting and a sort mode.  `Case.run()` steps the case on tests/track_ref.TrackChecker with verify=True — the
oracle pass by pass, its sort's permutation derived from the keys and checked against the records the oracle's sort leaves — once,
and keeps per step the records, the start indices, the keys before the sort and the permutation.  From these come the figures the
CPU companions assert:
    moved         per step, the share of slots whose occupant changes under the checker's permutation
    tie_slots     per step, the number of slots where the reference network's arrangement of the step's keys
                  (oracle.bitonic_keys) differs from the stable one (np.argsort(kind="stable")): where an id that followed the
                  wrong sort's tie order would show
    finite_after  per step, whether every float of the oracle's records is finite after it

Conditions (asserted in tests/test_tracking.py): a case of at least 64 particles has a step with moved > 0.5; a tie case run
with the reference network has a step with tie_slots > 0.  A case whose builder's upload order does not meet its condition on the
oracle is uploaded in a shuffled order instead (`p[rng.permutation(n)]`, `Case.shuffled`): the condition is never relaxed."""
import numpy as np

from tests import csort_scenes as CS
from tests import parity_states as PS
from tests import prologue_scenes as S
from tests.dense_scene import dense_scene

f32 = np.float32
FLOAT_FIELDS = ("position", "predicted_position", "velocity", "density")
SORTS = ("bitonic", "counting")
MIN_STEPS = 3
MOVED_MIN_N = 64                   # below it a handful of slots decides the share: no condition on `moved` there
SHUFFLE_SEED = 77
TIE_FAMILIES = ("coincident", "one_cell", "corners", "dense_scene", "strip")


class Step:
    """one checker step: records and start indices after it, the keys before the sort (in upload / previous slot order) and the
    permutation the sort applied (slot i holds what slot perm[i] held)"""

    def __init__(self, rec, start, keys, perm):
        self.rec, self.start, self.keys, self.perm = rec, start, keys, perm
        for a in (rec, start, keys, perm):
            a.setflags(write=False)


class Case:
    def __init__(self, name, st, off, tick, start, steps, quirks=True, sort="bitonic", field=None, start_indices=None):
        assert steps >= MIN_STEPS and sort in SORTS
        self.name, self.st, self.off, self.tick, self.steps = name, st, (float(off[0]), float(off[1])), tick, steps
        self.built = start
        self.start = start
        self.quirks, self.sort, self.field, self.start_indices = quirks, sort, field, start_indices
        self.family = name.split("/")[0]
        self.shuffled = False
        self.n = start.shape[0]
        self._run = None

    @property
    def stable(self):
        return self.sort == "counting"

    @property
    def tie_case(self):
        return self.family in TIE_FAMILIES

    def checker(self, channels=0, verify=False):
        from tests.track_ref import TrackChecker
        chk = TrackChecker(self.st, self.off, ref_quirks=self.quirks, channels=channels, verify=verify)
        chk.set_particles(self.start)
        if self.start_indices is not None:
            chk.start_indices_view()[:] = self.start_indices
        if self.field is not None:
            chk.sim.texture_view()[:] = self.field
        return chk

    def _steps(self):
        chk = self.checker(verify=True)
        out = []
        with np.errstate(all="ignore"):
            for _ in range(self.steps):
                perm = chk.step(self.tick, stable_sort=self.stable)
                rec = chk.particles()
                keys = np.empty(self.n, dtype=np.uint32)
                keys[perm] = rec["grid"]                    # the move pass leaves the keys the sort arranged
                out.append(Step(rec, chk.start_indices_view().copy(), keys, perm.copy()))
        chk.close()
        return out

    def _shuffle(self):
        self.start = self.built[np.random.default_rng(SHUFFLE_SEED).permutation(self.n)]
        self.shuffled = True

    def run(self):
        """the whole case on the checker: a list of Step, computed once.  The upload order is settled here: the builder's, or —
        where that misses the case's condition — the shuffled one."""
        if self._run is None:
            self._run = self._steps()
            if not self.shuffled and not self.meets_conditions():
                self._shuffle()
                self._run = self._steps()
        return self._run

    # ---- figures ----
    def moved(self):
        return [float((s.perm != np.arange(self.n)).mean()) for s in self.run()]

    def tie_slots(self):
        from oracle import oracle as O
        return [int((O.bitonic_keys(s.keys)[1] != np.argsort(s.keys, kind="stable")).sum()) for s in self.run()]

    def finite_after(self):
        return [bool(all(np.isfinite(s.rec[f]).all() for f in FLOAT_FIELDS)) for s in self.run()]

    @property
    def stays_finite(self):
        return all(self.finite_after())

    def meets_conditions(self):
        ok = self.n < MOVED_MIN_N or max(self.moved()) > 0.5
        if self.tie_case and not self.stable:
            ok = ok and max(self.tie_slots()) > 0
        return ok

    def ids(self):
        """the checker's ids after every step, from the enable's iota"""
        out, ids = [], np.arange(self.n, dtype=np.uint32)
        for s in self.run():
            ids = ids[s.perm]
            out.append(ids)
        return out

    def describe(self):
        return (f"[hard_states2d] {self.name} (n {self.n}, {self.sort}, quirks {int(self.quirks)}, shuffled {int(self.shuffled)}): "
                f"moved {[round(m, 3) for m in self.moved()]}, tie_slots {self.tie_slots()}, finite_after {[int(x) for x in self.finite_after()]}")


_CASES = {}


def _cached(key, build):
    if key not in _CASES:
        _CASES[key] = build()
    return _CASES[key]


# ---- the builders' states, assembled ----------------------------------------------------------------------------------------
def guard_case(fs, orc, name):
    """test_force_quotient_guards: 3 steps"""
    def build():
        st, off, tick, p = PS.jittered_dam_break(fs, orc, 4096, PS.GUARD_SEED, **PS.guard_overrides(name))
        return Case(f"guard/{name}", st, off, tick, PS.guard_state(orc, st, p, name), 3)
    return _cached(("guard", name), build)


def nan_clamp_case(fs, orc):
    """test_nan_reset_speed_clamp_and_walls: 4 steps"""
    def build():
        st, off, tick = PS.pair_settings(fs, 4096)
        p = PS.nan_clamp_state(PS.jitter(PS.lattice(orc, st, off), PS.NAN_CLAMP["seed"], PS.NAN_CLAMP["vel"]))
        return Case("nan_clamp", st, off, tick, p, 4)
    return _cached(("nan_clamp",), build)


def coincident_case(fs, orc):
    """test_coincident_particles_prng_path: 3 steps"""
    def build():
        st, off, tick, p = PS.jittered_dam_break(fs, orc, 4096, PS.COINCIDENT["seed"])
        return Case("coincident", st, off, tick, PS.coincident_state(p), 3)
    return _cached(("coincident",), build)


def mouse_field_case(fs, orc):
    """test_mouse_and_force_field: 5 steps"""
    def build():
        over = dict(PS.MOUSE_FIELD)
        seed = over.pop("seed")
        st, off, tick, p = PS.jittered_dam_break(fs, orc, 4096, seed, **over)
        return Case("mouse_field", st, off, tick, p, 5, field=PS.mouse_field())
    return _cached(("mouse_field",), build)


def dam_case(fs, orc, n):
    """test_ragged_counts of the plain suite: n particles in the 9 x 7 box, 4 steps"""
    def build():
        st, off, tick, p = PS.jittered_dam_break(fs, orc, n, n, size=PS.RAGGED_BOX)
        return Case(f"dam/{n}", st, off, tick, p, 4)
    return _cached(("dam", n), build)


def random_case(fs, orc, k, sort):
    """test_random_configurations: configuration k in the given sort mode (each mode has its own draw of the state), 4 steps.  The
    plain test runs them with quirks on; here, as in tests/features2d.py, odd k run with quirks off."""
    def build():
        st, off, tick, runs = PS.random_configuration(fs, orc, k)
        _, p, field = runs[SORTS.index(sort)]
        return Case(f"random/{k}/{sort}", st, off, tick, p, 4, quirks=k % 2 == 0, sort=sort, field=field)
    return _cached(("random", k, sort), build)


def dense_case(fs, orc, sort):
    def build():
        st, tick, p = dense_scene(fs)
        return Case(f"dense_scene/{sort}", st, (0.0, 0.0), tick, p, 3, sort=sort)
    return _cached(("dense", sort), build)


def corners_case(fs, orc, quirks, sort):
    def build():
        st, tick, p = S.corners()
        return Case(f"corners/{'quirks' if quirks else 'noquirks'}/{sort}", st, (0.0, 0.0), tick, p.copy(), 3, quirks=quirks, sort=sort)
    return _cached(("corners", quirks, sort), build)


def ragged_case(fs, orc, n, sort):
    def build():
        st, tick, p = S.ragged(n)
        return Case(f"ragged/{n}/{sort}", st, (0.0, 0.0), tick, p.copy(), 3, sort=sort)
    return _cached(("ragged", n, sort), build)


def staging_case(fs, orc, name, sort):
    """one_cell and the four strips of tests/prologue_scenes.py"""
    def build():
        st, tick, p = S.staging_scene(name)
        cid = f"one_cell/{sort}" if name == "one_cell" else f"strip/{name}/{sort}"
        return Case(cid, st, (0.0, 0.0), tick, p.copy(), 3, sort=sort)
    return _cached(("staging", name, sort), build)


# the scenes tests/test_csort_gpu.py runs as whole steps (assert_stable_step): name -> builder of (settings, tick, records, facts)
CSORT_SCENES = [(f"rank/{m}", lambda m=m, b=b, a=a: CS.one_cell(m, b, a)) for m, b, a in CS.RANK_CASES] + \
    [(f"placement/{m}/{b}", lambda m=m, b=b, a=a: CS.one_cell(m, b, a)) for m, b, a, _, _ in CS.PLACEMENT_CASES] + \
    [(f"two/{ma}/{mb}/{b}", lambda ma=ma, mb=mb, b=b: CS.two_cells(ma, mb, b)) for ma, mb, b, _ in CS.TWO_CASES] + \
    [(f"all/{n}", lambda n=n: CS.all_in_one(n)) for n in CS.ALL_CASES] + \
    [(f"lattice/{n}", lambda n=n: CS.lattice(n)) for n in CS.LATTICE_N] + \
    [(f"table/{gw}x{gh}", lambda gw=gw, gh=gh: CS.table(gw, gh)) for gw, gh, _, _ in CS.TABLE_CASES] + \
    [(f"runs/{pat}", lambda pat=pat: CS.runs(pat)) for pat in CS.RUN_PATTERNS]


def csort_case(fs, orc, name):
    def build():
        st, tick, p, _ = dict(CSORT_SCENES)[name]()
        return Case(f"csort/{name}", st, (0.0, 0.0), tick, p.copy(), 3, sort="counting")
    return _cached(("csort", name), build)


# ---- the registry -----------------------------------------------------------------------------------------------------------
def all_cases(fs, orc):
    """(id, builder) of every case, in the order the GPU files run them"""
    out = [(f"guard/{g}", lambda g=g: guard_case(fs, orc, g)) for g in PS.GUARD_CASES]
    out += [("nan_clamp", lambda: nan_clamp_case(fs, orc)), ("coincident", lambda: coincident_case(fs, orc)),
            ("mouse_field", lambda: mouse_field_case(fs, orc))]
    out += [(f"dam/{n}", lambda n=n: dam_case(fs, orc, n)) for n in PS.RAGGED_DAM_N]
    out += [(f"random/{k}/{s}", lambda k=k, s=s: random_case(fs, orc, k, s)) for k in range(PS.RANDOM_CASES) for s in SORTS]
    out += [(f"dense_scene/{s}", lambda s=s: dense_case(fs, orc, s)) for s in SORTS]
    out += [(f"corners/{'quirks' if q else 'noquirks'}/{s}", lambda q=q, s=s: corners_case(fs, orc, q, s))
            for q in (True, False) for s in SORTS]
    out += [(f"ragged/{n}/{s}", lambda n=n, s=s: ragged_case(fs, orc, n, s)) for n in S.RAGGED_N for s in SORTS]
    out += [(f"one_cell/{s}", lambda s=s: staging_case(fs, orc, "one_cell", s)) for s in SORTS]
    out += [(f"strip/{name}/{s}", lambda name=name, s=s: staging_case(fs, orc, name, s)) for name, _, _ in S.STRIP_CASES for s in SORTS]
    out += [(f"csort/{name}", lambda name=name: csort_case(fs, orc, name)) for name, _ in CSORT_SCENES]
    return out


CASE_IDS = [cid for cid, _ in all_cases(None, None)]
TIE_CASE_IDS = [cid for cid in CASE_IDS if cid.split("/")[0] in TIE_FAMILIES]


def case_by_id(fs, orc, cid):
    case = dict(all_cases(fs, orc))[cid]()
    assert case.name == cid
    return case


# ---- query points of the sampling tests -------------------------------------------------------------------------------------
def query_cells(st, pts):
    """(cx, cy) of every point by the statement of include/fluidsim.h (tests/pyref.py's xy_of_point: f32, true division,
    u32_sat, wrapping + 1) — not through the sampler under test"""
    from tests import pyref
    u = {"bounds": (f32(st.size.x), f32(st.size.y)), "h": f32(st.smoothing_radius)}
    with np.errstate(all="ignore"):
        return np.array([pyref.xy_of_point(u, pt) for pt in np.asarray(pts, dtype=f32)], dtype=np.int64).reshape(-1, 2)


def special_queries(st, p):
    """The points at which the cell coordinates of a query saturate, wrap or leave the grid, for a state `p` (records after a
    step) in a box (sx, sy) with cell side h: the `boundaries` set of tests/test_sampling_gpu.py (cell boundaries, the box's
    corners); x = +-sx/2 and y = +-sy/2 and one f32 ulp either side; the centres of the cells of columns grid_w - 2 ..
    grid_w + 1 (one valid column at grid_w, none at grid_w + 1) and rows grid_h - 2 .. grid_h + 1, against each other and against
    the first and a middle column / row; (+-1e10, 0), (0, +-1e10) and +-3e38, whose quotient saturates or overflows; +-inf
    and NaN in either coordinate and in both; +-0.0; and points whose column wraps to 0 (u32_sat(..) + 1) in a valid row —
    next to the fluid's own rows — with the transpose."""
    from tests.test_sampling_gpu import query_sets
    sx, sy, h = float(st.size.x), float(st.size.y), float(st.smoothing_radius)
    gw, gh = CS.formula_grid(st)
    inf, nan = np.inf, np.nan
    out = [query_sets(st, p, np.random.default_rng(0))["boundaries"]]
    ex = [np.nextafter(f32(s * sx / 2), f32(d)) for s in (-1, 1) for d in (-inf, inf)] + [f32(-sx / 2), f32(sx / 2)]
    ey = [np.nextafter(f32(s * sy / 2), f32(d)) for s in (-1, 1) for d in (-inf, inf)] + [f32(-sy / 2), f32(sy / 2)]
    own = p["predicted_position"]
    ys = [0.0, float(own[0, 1]), float(own[-1, 1]), -sy / 4]
    xs = [0.0, float(own[0, 0]), float(own[-1, 0]), sx / 4]
    out.append([(x, y) for x in ex for y in ys + ey])
    out.append([(x, y) for y in ey for x in xs])
    cols = [1, 2, gw // 2] + list(range(gw - 2, gw + 2))
    rows = [1, 2, gh // 2] + list(range(gh - 2, gh + 2))
    out.append([((c - 0.5) * h - sx / 2, (r - 0.5) * h - sy / 2) for c in cols for r in rows])
    far = [1e10, -1e10, 3e38, -3e38, inf, -inf, nan]
    out.append([(v, y) for v in far for y in ys + [(r - 0.5) * h - sy / 2 for r in (1, gh - 1)]])
    out.append([(x, v) for v in far for x in xs + [(c - 0.5) * h - sx / 2 for c in (1, gw - 1)]])
    out.append([(a, b) for a in far for b in far])
    out.append([(0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0)])
    return np.concatenate([np.asarray(o, dtype=np.float64).reshape(-1, 2) for o in out]).astype(f32)


UNIFORM_QUERIES = 16000            # the sparsest scene (129 particles in two cells of a 40 x 30 box) is hit by one point in 3000


def uniform_queries(st, seed=5):
    """points drawn uniformly over 1.2 x the box: they must both hit and miss the fluid"""
    rng = np.random.default_rng(seed)
    sx, sy = float(st.size.x), float(st.size.y)
    return np.stack([rng.uniform(-0.6 * sx, 0.6 * sx, UNIFORM_QUERIES), rng.uniform(-0.6 * sy, 0.6 * sy, UNIFORM_QUERIES)], axis=1).astype(f32)


def sample_channel_values(n, channels, seed=31):
    """finite channel values that include +-0.0, denormals and large magnitudes (1e30: the sums stay finite) — a skipped
    candidate is a branch in the sampler, not an added zero, and a -0.0 sum shows the difference"""
    rng = np.random.default_rng(seed)
    pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -3e-39, 1.0, -1.0, 1e30, -1e30, 0.3, -2.5e-7], dtype=f32)
    out = pool[rng.integers(0, pool.size, size=(channels, n))]
    if channels > 1:
        out[1] = f32(-0.0)                                         # a channel of negative zeros: its sums are -0 terms only
    return np.ascontiguousarray(out)
