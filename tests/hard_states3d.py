"""The hard inputs of the plain 3D step, as ONE registry for everything that reads the 3D state after a step: the field sampler
(k3_sample, k3_sample_attr), the two walks of csrc/fs_field3.h behind the ray-marcher and the surface extractor, and the tracking
carry behind k3_reorder (tests/test_3d_queries_hard_inputs_gpu.py; CPU companion tests/test_hard_states3d.py).  TEST
INFRASTRUCTURE ONLY: plain numpy on the unchanged 3D oracle, no GPU.

The states are those of the plain tests, taken from their builders (tests/paths3d.py, and the three own guard states of
tests/features3d.py with the features off): the operand guards, the six smoothing radii, twelve seeded random boxes with their
drawn offsets, particles on and far outside every face, edge and corner, the block driven into each wall, the one-cell and the
three-cells-thin grids, and two path scenes with over-full cells.  No state is copied.

A case is a name, settings, an offset, a tick, start records and a number of steps.  `Case.run()` steps the case on
oracle.OracleSim3D once and keeps the records after every step (read-only); `stays_finite` is read off them.

Also here: the query points at which a query's cell coordinates saturate, wrap or leave the grid (special_queries3), the header's
cell expression for them (query_cells3, query_cell_ids3), and the two lists the CPU companion verifies against the oracle:
TIE_CASE_IDS (two records share a key after a step) and ONE_KEY_CASE_IDS (all records share ONE key after every step)."""
import numpy as np

import paths3d
from tests import features3d as F3
from tests.track3d_ref import cell_xyz

f32 = np.float32
FLOAT_FIELDS = ("position", "predicted_position", "velocity", "density")
RANDOM_CASES = 12                  # seeds 0..11 of paths3d.random_case: every `case % 4` shape three times
SCENE_LONGEST_ROW = F3.LONGEST_ROW                 # "row129": one cell of 129 particles, the chunked sweep
SCENE_COINCIDENT = "coincident_two_word"           # 110 particles in one cell, five of them at one point
SCENES = (SCENE_LONGEST_ROW, SCENE_COINCIDENT)


class Case:
    def __init__(self, orc, name, st, off, tick, start, steps):
        self.orc, self.name, self.st, self.tick, self.steps = orc, name, st, tick, steps
        self.off = tuple(float(x) for x in off)
        self.start = start
        self.start.setflags(write=False)
        self.n = start.shape[0]
        self.h = float(st.smoothing_radius)
        self._run = None
        self.grid_dims = grid_dims3(st)

    def run(self):
        """the plain oracle's records after every step: a list of `steps` read-only arrays, computed once"""
        if self._run is None:
            ref = self.orc.OracleSim3D(self.st, self.off)
            ref.set_particles(self.start)
            out = []
            with np.errstate(all="ignore"):
                for _ in range(self.steps):
                    ref.step(self.tick)
                    rec = ref.particles()
                    rec.setflags(write=False)
                    out.append(rec)
            self.constants = ref.constants()                            # (poly6, ...) as the oracle's step evaluates them
            ref.close()
            self._run = out
        return self._run

    def finite_after(self):
        return [bool(all(np.isfinite(rec[fld]).all() for fld in FLOAT_FIELDS)) for rec in self.run()]

    @property
    def stays_finite(self):
        return all(self.finite_after())

    @property
    def ncell(self):
        return self.grid_dims[0] * self.grid_dims[1] * self.grid_dims[2]

    def shares_a_key(self):
        """per step: at least two records share a key"""
        return [bool((np.diff(rec["grid"].astype(np.int64)) == 0).any()) for rec in self.run()]

    def one_key(self):
        """per step: all records share one key — the sort's network then swaps nothing, and the statement is "nothing moves\""""
        return [bool((rec["grid"] == rec["grid"][0]).all()) for rec in self.run()]


# ---- the builders' states, assembled ----------------------------------------------------------------------------------------
_CASES = {}
ZERO = (0.0, 0.0, 0.0)


def _cached(key, build):
    if key not in _CASES:
        _CASES[key] = build()
    return _CASES[key]


def guard_case(fs, orc, name):
    """test_3d_force_quotient_guards, and the three own guard states of tests/features3d.py with the features off: 3 steps"""
    def build():
        own = {"mass_tiny": F3._mass_tiny, "positions_on_plus_b": F3._positions_on_plus_b, "nan_next_to_everyone": F3._nan_next_to_everyone}
        if name in own:
            st, tick, p = own[name](fs, orc)
        else:
            ref, st, tick, p = paths3d.pair3_state(fs, orc, 12, **paths3d.guard_overrides(name))
            ref.close()
            p = paths3d.guard_state(orc, st, p, name)
            p["predicted_position"] = p["position"]                      # as run3 uploads it
        return Case(orc, f"guard/{name}", st, ZERO, tick, p, 3)
    return _cached(("guard", name), build)


def radius_case(fs, orc, h):
    def build():
        ref, st, tick, p = paths3d.radius_state(fs, orc, h)
        ref.close()
        return Case(orc, f"radius/{h}", st, ZERO, tick, p, 3)
    return _cached(("radius", h), build)


def random_case(fs, orc, k):
    def build():
        st, off, tick, mutate, _ = paths3d.random_case(fs, k)
        ref = orc.OracleSim3D(st, off)
        p = mutate(ref.particles())
        ref.close()
        return Case(orc, f"random/{k}", st, off, tick, p, 4)
    return _cached(("random", k), build)


def faces_case(fs, orc, which):
    def build():
        st, tick, p = paths3d.faces_state(fs, orc, which == "exact")
        return Case(orc, f"faces/{which}", st, ZERO, tick, p, 4)
    return _cached(("faces", which), build)


def wall_name(axis, sign):
    return f"wall/{axis}{'+' if sign > 0 else '-'}"


def wall_case(fs, orc, axis, sign):
    def build():
        ref, st, tick, p = paths3d.wall_state(fs, orc, axis, sign)
        ref.close()
        return Case(orc, wall_name(axis, sign), st, ZERO, tick, p, 4)
    return _cached(("wall", axis, sign), build)


def thin_case(fs, orc, i):
    def build():
        st, tick, p = paths3d.thin_state(fs, orc, paths3d.THIN_SIZES[i])
        return Case(orc, f"thin/{i}", st, ZERO, tick, p, 3)
    return _cached(("thin", i), build)


def scene_case(fs, orc, name):
    def build():
        scene = paths3d.scenes()[name]
        st, tick, p = paths3d.build_state(fs, scene)
        return Case(orc, f"scene/{name}", st, ZERO, tick, p, scene.steps)
    return _cached(("scene", name), build)


# ---- the registry -----------------------------------------------------------------------------------------------------------
def all_cases(fs, orc):
    """(id, builder) of every case, in the order the GPU file runs them"""
    out = [(f"guard/{g}", lambda g=g: guard_case(fs, orc, g)) for g in F3.GUARDS]
    out += [(f"radius/{h}", lambda h=h: radius_case(fs, orc, h)) for h in paths3d.RADII]
    out += [(f"random/{k}", lambda k=k: random_case(fs, orc, k)) for k in range(RANDOM_CASES)]
    out += [(f"faces/{w}", lambda w=w: faces_case(fs, orc, w)) for w in ("exact", "inexact")]
    out += [(wall_name(a, s), lambda a=a, s=s: wall_case(fs, orc, a, s)) for a, s in paths3d.WALLS]
    out += [(f"thin/{i}", lambda i=i: thin_case(fs, orc, i)) for i in range(len(paths3d.THIN_SIZES))]
    out += [(f"scene/{s}", lambda s=s: scene_case(fs, orc, s)) for s in SCENES]
    return out


CASE_IDS = [cid for cid, _ in all_cases(None, None)]

# the cases whose oracle records hold a non-finite float after some step (tests/test_hard_states3d.py asserts the list)
NOT_FINITE_CASE_IDS = ["guard/inf_velocity", "guard/huge_pressure", "guard/unsafe_next_to_safe", "guard/nan_next_to_everyone"]
# at least two records share a key after a step: with more particles than occupied cells, every case of the registry
TIE_CASE_IDS = list(CASE_IDS)
# ... and all records share ONE key after every step: the whole box is one cell
ONE_KEY_CASE_IDS = ["guard/nan_next_to_everyone", "thin/0"]
# the cases of the renderer and the extractor: the radii, the thin grids, the faces, two guards and two offset boxes
SURFACE_CASE_IDS = [f"radius/{h}" for h in paths3d.RADII] + [f"thin/{i}" for i in range(len(paths3d.THIN_SIZES))] + \
    ["faces/exact", "faces/inexact", "guard/density_across_2p20", "guard/mass_tiny", "random/1", "random/2"]
TOLERANCE_CASE_IDS = ["radius/0.05", "radius/1.0", "thin/0", "faces/exact", "guard/density_across_2p20"]


def case_by_id(fs, orc, cid):
    case = dict(all_cases(fs, orc))[cid]()
    assert case.name == cid
    return case


# ---- query points -------------------------------------------------------------------------------------------------------------
def query_cells3(st, pts):
    """(cx, cy, cz) of every point by the statement of include/fluidsim.h (f32, true division, u32_sat, wrapping + 1): (n, 3)
    uint32 — tests/track3d_ref.cell_xyz, not the sampler under test"""
    with np.errstate(all="ignore"):
        return cell_xyz(st, np.asarray(pts, dtype=f32).reshape(-1, 3))


def query_cell_ids3(st, grid_dims, pts):
    """cell = (cz * grid_h + cy) * grid_w + cx, wrapping u32"""
    c = query_cells3(st, pts).astype(np.uint64)
    gw, gh = np.uint64(grid_dims[0]), np.uint64(grid_dims[1])
    return (((c[:, 2] * gh + c[:, 1]) * gw + c[:, 0]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _half(st):
    return f32([st.size.x, st.size.y, st.size.z]) * f32(0.5)


def _finite_rows(a):
    a = np.asarray(a, dtype=f32).reshape(-1, 3)
    return a[np.isfinite(a).all(axis=1)]


def special_queries3(st, p):
    """The points at which the cell coordinates of a query saturate, wrap or leave the grid, for a state `p` (records after a
    step) in a box of half extents b with cell side h.  Per axis a, with the other two coordinates taken from `anchors` (the
    origin, the first record, the last record, the record nearest the +b wall and the one nearest the -b wall of that axis, so
    that the point lies in rows the fluid occupies):
      - exactly -b and +b, and one f32 ulp either side of each
      - the centres of the cells grid_a - 2 .. grid_a + 1 (one valid column at grid_a, none at grid_a + 1) and of cells 1 and 2
      - 2^32 h, 2^33 h and 3e38: the quotient saturates (or overflows) and the + 1 wraps the cell coordinate to 0
      - -(b + 5 h), -1e10 and -3e38: far below -b, where u32_sat gives 0 and the cell coordinate is 1
    and: the 8 corners, 12 edge mid-points and 6 face centres of the box; the same 26 points with 2^32 h in place of b (all
    three coordinates wrap at once); the cell-boundary points of tests/sample3d_ref.boundary_points; the positions of the
    records in the first and in the last occupied cell; points next to every record whose key lies past the cell table.
    No non-finite coordinate: the header leaves those unspecified (records with a non-finite position are skipped as anchors)."""
    from tests.sample3d_ref import boundary_points
    h = f32(st.smoothing_radius)
    b = _half(st)
    ref = grid_dims3(st)
    own = _finite_rows(p["predicted_position"])
    assert own.shape[0] >= 2, "no finite record to anchor the queries on"
    inf = f32(np.inf)
    out = []
    big = f32(4294967296.0) * h
    for a in range(3):
        anchors = [np.zeros(3, f32), own[0], own[-1], own[np.argmax(own[:, a])], own[np.argmin(own[:, a])]]
        g = ref[a]
        vals = [-b[a], b[a]] + [np.nextafter(s * b[a], d) for s in (f32(-1), f32(1)) for d in (-inf, inf)]
        vals += [(f32(c) - f32(0.5)) * h - b[a] for c in (1, 2, g - 2, g - 1, g, g + 1)]
        vals += [big, f32(2) * big, f32(3e38)]
        vals += [-(b[a] + f32(5) * h), f32(-1e10), f32(-3e38)]
        for v in vals:
            for anchor in anchors:
                q = anchor.copy()
                q[a] = v
                out.append(q)
    signs = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if (x, y, z) != (0, 0, 0)]
    out += [f32(s) * b for s in signs]
    out += [np.where(f32(s) > 0, big, np.where(f32(s) < 0, -big, f32(0))).astype(f32) for s in signs]
    pts = [np.array(out, dtype=f32)]
    finite = p[np.isfinite(p["predicted_position"]).all(axis=1)]
    pts.append(boundary_points(st, finite, min(60, finite.shape[0]), seed=3))
    grid = p["grid"]
    pts.append(p["predicted_position"][grid == grid[0]])
    pts.append(p["predicted_position"][grid == grid[-1]])
    past = p["predicted_position"][grid >= np.uint32(min(ref[0] * ref[1] * ref[2], 0xFFFFFFFF))]
    if past.shape[0]:
        pts.append(past)
        pts.append(past + f32(0.25) * h)
        pts.append(past - f32(0.25) * h)
    return _finite_rows(np.concatenate([np.asarray(q, dtype=f32).reshape(-1, 3) for q in pts]))


def grid_dims3(st):
    """(grid_w, grid_h, grid_d) of a settings record, from the oracle"""
    from oracle import oracle as O
    ref = O.OracleSim3D(st)
    dims = ref.grid_dims
    ref.close()
    return dims


def nan_records(out):
    """per fs3_sample record: one of its floats is a NaN"""
    return np.isnan(out["density"]) | np.isnan(out["weight"]) | np.isnan(out["velocity"]).any(axis=-1) | np.isnan(out["gradient"]).any(axis=-1)


UNIFORM_QUERIES = 4000


def uniform_queries3(st, seed=2, count=UNIFORM_QUERIES):
    """points drawn uniformly over 1.2 x the box (tests/sample3d_ref.uniform_points): they must both hit and miss the fluid"""
    from tests.sample3d_ref import uniform_points
    return uniform_points(st, count, seed=seed)


def query_sets3(st, p, finite_only=False):
    """{name: points}: own (the records' predicted positions, slot order), shuffled, special, uniform.  finite_only: own and
    shuffled keep the finite points alone (a non-finite query coordinate is unspecified)."""
    own = p["predicted_position"].copy()
    if finite_only:
        own = _finite_rows(own)
    rng = np.random.default_rng(1)
    return {"own": own, "shuffled": own[rng.permutation(own.shape[0])], "special": special_queries3(st, p),
            "uniform": uniform_queries3(st)}


# ---- the renderer and the extractor ---------------------------------------------------------------------------------------------
RENDER_SIZES = [(37, 23), (1, 65)]         # ragged against the 8 x 8 wave tile and the 16 x 16 workgroup; one column
REFINES = (0, 8)
MARCH_STEPS = 64                           # of h / 2
LATTICES = [(2, 2, 2), (5, 4, 3), (17, 9, 6), (33, 33, 33)]
LARGEST = (33, 33, 33)


def surface_renders(st, p):
    """(context, camera, params) of every render of a state: tests/render3d_ref.scene_cameras at RENDER_SIZES, refine 0 and 8,
    iso_of(p), 64 steps of h / 2"""
    from tests.render3d_ref import iso_of, params, scene_cameras
    iso = iso_of(p)
    for w, hh in RENDER_SIZES:
        for name, (cam, t_near) in scene_cameras(st, p, w, hh).items():
            for refine in REFINES:
                yield f"{name} {w}x{hh} refine {refine}", cam, params(iso, t_near, 0.5 * st.smoothing_radius, MARCH_STEPS, refine)


def surface_meshes(st, p):
    """(context, lattice, world_min, world_max, iso) of every extraction of a state: tests/mesh3d_ref.scene_views at LATTICES"""
    from tests.mesh3d_ref import scene_views
    from tests.render3d_ref import iso_of
    iso = iso_of(p)
    for name, (wmin, wmax) in scene_views(st, p).items():
        for dims in LATTICES:
            yield f"view {name} lattice {dims}", dims, wmin, wmax, iso


# ---- a candidate exactly on the radius --------------------------------------------------------------------------------------------
# `if not (r2 > h2)` admits r2 == h2, where W is exactly 0.  In a finite state such a candidate adds +-0 to sums that start at +0
# and changes no bit of them, so only a state with a non-finite velocity shows whether the full-sample walk of csrc/fs_field3.h
# admits it: the term 0 * NaN is a NaN.  guard/huge_pressure after its first step holds records with a NaN velocity, a finite
# position and a finite density.
PROBE_CASE_ID, PROBE_STEP = "guard/huge_pressure", 1


def _r2(pj, q):
    """the statement's r2 of record position pj seen from q: f32, one rounding per operation, this association"""
    d = pj - q
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def radius_probe(st, p, sample, iso, seed=17, directions=40):
    """(q, beyond, j): a point q at exactly h from record j (r2 == h2 in the statement's f32 arithmetic), j's velocity not
    finite, such that by `sample` (a checker's) the density at q reaches `iso`, the velocity sum at q is a NaN, and at `beyond` —
    q moved outwards by ulps of one coordinate until r2 > h2 — every sum is finite: record j alone decides.  q is searched
    along seeded directions that point towards the fluid's centre, one coordinate stepped ulp by ulp across the sphere: along
    the direction's smallest component a step changes r2 by less than its own ulp, so no value of r2 is skipped.
    None when the state has no such point."""
    h = f32(st.smoothing_radius)
    h2 = h * h
    pos = p["predicted_position"]
    ok = np.isfinite(pos).all(axis=1)
    centre = pos[ok].mean(axis=0)
    cand = np.flatnonzero(~np.isfinite(p["velocity"]).all(axis=1) & ok & np.isfinite(p["density"]))
    rng = np.random.default_rng(seed)
    for j in cand:
        for _ in range(directions):
            u = np.abs(rng.standard_normal(3)) * np.sign(centre - pos[j])
            u[rng.integers(0, 3)] *= 0.05                                  # one small component: the one that is stepped
            u /= np.linalg.norm(u)
            a = int(np.argmin(np.abs(u)))
            away = f32(np.inf) * f32(np.sign(u[a]) or 1.0)
            q = (pos[j] + f32(0.99999) * h * u.astype(f32)).astype(f32)    # just inside the sphere
            for _ in range(4000):
                if not _r2(pos[j], q) < h2:
                    break
                q[a] = np.nextafter(q[a], away)
            if _r2(pos[j], q) != h2:
                continue
            beyond = q.copy()
            for _ in range(4000):
                if _r2(pos[j], beyond) > h2:
                    break
                beyond[a] = np.nextafter(beyond[a], away)
            if not _r2(pos[j], beyond) > h2:
                continue
            with np.errstate(all="ignore"):
                at = sample(np.stack([q, beyond]))
            if at["density"][0] >= f32(iso) and at["density"][1] >= f32(iso) and np.isnan(at["velocity"][0]).any() and not nan_records(at)[1]:
                return q, beyond, int(j)
    return None


def probe_renders(st, q, beyond, iso):
    """((camera, params), (camera, params)): one parallel ray starting AT q and one at `beyond` — a 1 x 1 orthographic image has
    u = v = 0, so o = eye, and with t_near = 0 the first sample is x(0) = o: the ray starts inside (hit == 2) and the full sample
    runs at exactly that point"""
    from tests.render3d_ref import camera, params
    sp = params(iso, 0.0, 0.5 * st.smoothing_radius, MARCH_STEPS, 0)
    return [(camera(x, [0, 0, 1], [1, 0, 0], [0, 1, 0], 1, 1, True), sp) for x in (q, beyond)]


# ---- the offset scan with real work ---------------------------------------------------------------------------------------------
SCAN_SIDE, SCAN_STEPS = 18, 8
SCAN_WORKGROUP, SCAN_THREADS = 256, 1024   # B3M and B3M_SCAN of csrc/kernels_mesh3d.hip
SCAN_LATTICES = [((65, 65, 65), 1073, 2), ((129, 129, 65), 4226, 5)]      # lattice, workgroup sums, sums per scan thread


def scan_scene(fs):
    """(settings, offset, tick, start records): the 18^3 dam break with jittered velocities, as tests/test_mesh3d_gpu.py runs it"""
    from oracle import oracle as O
    from tests.track_ref import jitter_velocities
    st, off, tick = fs.dam_break_3d(SCAN_SIDE ** 3)
    ref = O.OracleSim3D(st, off)
    start = jitter_velocities(ref.particles(), 7)
    ref.close()
    return st, off, tick, start


def scan_view(st, p):
    """(world_min, world_max): from 2 h below the fluid's lowest corner to its median particle.  The view ENDS inside the fluid, so
    the mesh is open at the high faces and the last z-planes of the lattice — the nodes from 256 * 1024 on, whose workgroup sums
    only a scan with chunk > 1 reaches — hold vertices."""
    h = float(st.smoothing_radius)
    q = p["predicted_position"].astype(np.float64)
    wmin, wmax = q.min(axis=0) - 2 * h, np.median(q, axis=0)
    return tuple(float(f32(x)) for x in wmin), tuple(float(f32(x)) for x in wmax)


def vertex_nodes(dims, cells):
    """the node index (k * H + j) * W + i of the low corner of every vertex's cell — the kernels' linear order — from the checker's
    cell index (k * (H - 1) + j) * (W - 1) + i"""
    W, H, _ = dims
    c = np.asarray(cells, dtype=np.int64)
    i, r = c % (W - 1), c // (W - 1)
    return ((r // (H - 1)) * H + r % (H - 1)) * W + i


def scan_figures(dims, cells):
    """what the scan test asserts on the checker's mesh: the number of workgroup sums and of sums per scan thread, the vertices at
    nodes from 256 * 1024 on, and the vertices in even and in odd workgroups"""
    q = vertex_nodes(dims, cells)
    nwg = (dims[0] * dims[1] * dims[2] + SCAN_WORKGROUP - 1) // SCAN_WORKGROUP
    wg = q // SCAN_WORKGROUP
    return {"nwg": nwg, "chunk": (nwg + SCAN_THREADS - 1) // SCAN_THREADS, "far": int((q >= SCAN_WORKGROUP * 1024).sum()),
            "even": int((wg % 2 == 0).sum()), "odd": int((wg % 2 == 1).sum())}
