"""ctypes loader of the 3D surface-extraction checker (tests/mesh3d_checker.cpp on top of tests/sample3d_checker.cpp and
oracle/sph_oracle3d.cpp, both included unchanged).  TEST INFRASTRUCTURE ONLY.  Built and loaded on first use by
tests/checker_lib.py: the oracle's flags, a per-user cache outside the tree, keyed by the sources' contents.  Also here: a
numpy-f32 restatement of the statement (include/fluidsim.h "3D surface extraction") that shares no code with the checker, the
mask arithmetic that ties the counts to a sampled density volume, and the views the CPU and the GPU tests share."""
import ctypes as C

import numpy as np

from tests import checker_lib as CL
from tests import sample3d_ref as S3

P = C.c_void_p
SOURCES = [CL.here("mesh3d_checker.cpp")] + S3.SOURCES
OWN = {k: S3.OWN[k] for k in ("smp3_load", "smp3_sample", "smp3_sample_grid")}
OWN["msh3_extract"] = (None, [P, P, C.c_float, P, C.c_uint32, P, C.c_uint32, P, P, P])

MESH_VERTEX_DTYPE = np.dtype([("position", "<f4", (3,)), ("normal", "<f4", (3,)), ("velocity", "<f4", (3,)), ("density", "<f4")])
assert MESH_VERTEX_DTYPE.itemsize == 40
f = np.float32


class Vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class MeshVertex3(C.Structure):
    _fields_ = [("position", Vec3), ("normal", Vec3), ("velocity", Vec3), ("density", C.c_float)]


assert C.sizeof(MeshVertex3) == 40


def lib():
    return CL.load("mesh3d_checker", SOURCES, "orc3_", OWN)


class Mesh3Checker(S3.Sample3Checker):
    """The sampling checker with the surface nets of DESIGN.md §17 on the loaded state."""

    def __init__(self, settings, initial_offset=(0.0, 0.0, 0.0)):
        self.L = lib()
        self.settings = settings
        self.h = self.L.orc3_create(C.addressof(settings), *[float(x) for x in initial_offset])
        if not self.h:
            raise ValueError("checker: invalid settings")
        self.n = int(self.L.orc3_count(self.h))

    def extract(self, dims, wmin, wmax, iso, vert_cap=None, tri_cap=None, detail=False):
        """-> (vertices, triangles, (V, T)); the arrays hold min(count, cap) entries (no cap: everything).  detail=True adds the
        cell index and the local position of every vertex."""
        v = S3._view(dims[0], dims[1], dims[2], wmin, wmax)
        counts = np.zeros(2, dtype=np.uint32)
        if vert_cap is None or tri_cap is None:
            self.L.msh3_extract(self.h, C.addressof(v), float(iso), None, 0, None, 0, counts.ctypes.data, None, None)
            vert_cap = int(counts[0]) if vert_cap is None else vert_cap
            tri_cap = int(counts[1]) if tri_cap is None else tri_cap
        verts = np.zeros(vert_cap, dtype=MESH_VERTEX_DTYPE)
        tris = np.zeros((tri_cap, 3), dtype=np.uint32)
        cells = np.zeros(vert_cap, dtype=np.uint32)
        local = np.zeros((vert_cap, 3), dtype=np.float32)
        self.L.msh3_extract(self.h, C.addressof(v), float(iso), verts.ctypes.data, vert_cap, tris.ctypes.data, tri_cap,
                            counts.ctypes.data, cells.ctypes.data, local.ctypes.data)
        V, T = int(counts[0]), int(counts[1])
        out = (verts[:min(V, vert_cap)], tris[:min(T, tri_cap)], (V, T))
        return out + (cells[:min(V, vert_cap)], local[:min(V, vert_cap)]) if detail else out


# ---- views shared by the CPU and the GPU tests ----------------------------------------------------------------------------------
def scene_views(settings, particles):
    """{name: (world_min, world_max)} around the state's fluid."""
    h = float(settings.smoothing_radius)
    half = 0.5 * np.float64([settings.size.x, settings.size.y, settings.size.z])
    p = particles["predicted_position"]
    lo, hi = p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)
    out = {}
    out["overhang"] = (-half - 2 * h, half + 2 * h)                 # the whole domain and 2 h more on every side
    out["cut"] = (lo + 0.3 * (hi - lo), hi + 2 * h)                 # starts inside the fluid: the mesh is open at the low faces
    out["outside"] = (half + 3 * h, 3 * half + 3 * h)               # beyond the +x +y +z corner, farther than h from anything
    out["flip_x"] = ((half[0] + 2 * h, -half[1] - 2 * h, -half[2] - 2 * h), (-half[0] - 2 * h, half[1] + 2 * h, half[2] + 2 * h))
    return {k: (tuple(float(f(x)) for x in a), tuple(float(f(x)) for x in b)) for k, (a, b) in out.items()}


# ---- mask arithmetic on a density volume [D, H, W] ------------------------------------------------------------------------------
def active_cells(inside):
    """[D-1, H-1, W-1] bool: the cells whose eight corners are neither all inside nor all outside."""
    n = np.zeros(tuple(s - 1 for s in inside.shape), dtype=np.int32)
    D, H, W = inside.shape
    for c in (0, 1):
        for b in (0, 1):
            for a in (0, 1):
                n += inside[c:D - 1 + c, b:H - 1 + b, a:W - 1 + a]
    return (n != 0) & (n != 8)


def crossing_edges(inside, axis):
    """Interior lattice edges along `axis` (0 x, 1 y, 2 z) whose ends differ: (k, j, i) of their low nodes as an [E, 3] array in
    ascending node order, and whether the low node is inside."""
    ax = 2 - axis                                       # the array axis: volumes are [z, y, x]
    lo = np.take(inside, np.arange(inside.shape[ax] - 1), axis=ax)
    hi = np.take(inside, np.arange(1, inside.shape[ax]), axis=ax)
    cross = lo != hi
    for other in range(3):
        if other != ax:                                  # u and v: 1 .. extent - 2
            idx = np.arange(cross.shape[other])
            keep = (idx >= 1) & (idx <= inside.shape[other] - 2)
            cross &= keep.reshape([-1 if a == other else 1 for a in range(3)])
    at = np.argwhere(cross)
    return at, lo[cross]


def boundary_is_outside(inside):
    """The closedness condition: no node of the lattice's six boundary faces is inside."""
    return not (inside[0].any() or inside[-1].any() or inside[:, 0].any() or inside[:, -1].any() or inside[:, :, 0].any() or inside[:, :, -1].any())


def directed_edges_balance(tris):
    """Every directed triangle edge (a, b) occurs exactly as often as (b, a)."""
    t = np.asarray(tris, dtype=np.int64)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    n = int(t.max()) + 1 if t.size else 1
    a, ca = np.unique(e[:, 0] * n + e[:, 1], return_counts=True)
    b, cb = np.unique(e[:, 1] * n + e[:, 0], return_counts=True)
    return np.array_equal(a, b) and np.array_equal(ca, cb)


# ---- the numpy-f32 restatement --------------------------------------------------------------------------------------------------
# the twelve edges of a cell in the statement's order: (axis, low corner (x, y, z))
EDGES = [(0, (0, 0, 0)), (0, (0, 1, 0)), (0, (0, 0, 1)), (0, (0, 1, 1)),
         (1, (0, 0, 0)), (1, (1, 0, 0)), (1, (0, 0, 1)), (1, (1, 0, 1)),
         (2, (0, 0, 0)), (2, (1, 0, 0)), (2, (0, 1, 0)), (2, (1, 1, 0))]


def numpy_extract(sample, dims, wmin, wmax, iso):
    """(vertices, triangles[T, 3]) of the statement in np.float32.  `sample(x)` gives the sampling statement's sums at a point as
    a dict (density, weight, gradient[3], velocity[3]).  Vertices come from a table of edges, faces from array masks sorted by
    their order key: neither is the checker's loop."""
    W, H, D = dims
    iso = f(iso)
    ext = (W, H, D)
    ax = [f(wmin[a]) + ((np.arange(ext[a], dtype=f) + f(0.5)) / f(ext[a])) * (f(wmax[a]) - f(wmin[a])) for a in range(3)]
    assert all(a.dtype == f for a in ax)
    F = np.zeros((D, H, W), dtype=f)
    for k in range(D):
        for j in range(H):
            for i in range(W):
                F[k, j, i] = sample(f([ax[0][i], ax[1][j], ax[2][k]]))["density"]
    inside = F >= iso
    cells = np.argwhere(active_cells(inside))            # ascending (k, j, i): the vertex order
    rank = -np.ones((D - 1, H - 1, W - 1), dtype=np.int64)
    verts = np.zeros(len(cells), dtype=MESH_VERTEX_DTYPE)
    with np.errstate(all="ignore"):
        for r, (k, j, i) in enumerate(cells):
            rank[k, j, i] = r
            s, c = [f(0), f(0), f(0)], 0
            for axis, lo in EDGES:
                hi = list(lo)
                hi[axis] = 1
                Fa, Fb = F[k + lo[2], j + lo[1], i + lo[0]], F[k + hi[2], j + hi[1], i + hi[0]]
                if (Fa >= iso) == (Fb >= iso):
                    continue
                c += 1
                for a in range(3):
                    s[a] = s[a] + ((iso - Fa) / (Fb - Fa) if a == axis else f(lo[a]))
            idx = (i, j, k)
            pos = f([ax[a][idx[a]] + (s[a] / f(c)) * (ax[a][idx[a] + 1] - ax[a][idx[a]]) for a in range(3)])
            S = sample(pos)
            g = S["gradient"]
            gl = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            normal = [(-a) / gl for a in g] if gl > 0 else [f(0)] * 3
            vel = [a / S["weight"] for a in S["velocity"]] if S["weight"] > 0 else [f(0)] * 3
            verts[r] = (pos, normal, vel, S["density"])
    keys, quads = [], []
    for axis in range(3):
        at, low_in = crossing_edges(inside, axis)
        u, v = (axis + 1) % 3, (axis + 2) % 3
        for (k, j, i), lin in zip(at, low_in):
            n = [i, j, k]

            def cell(du, dv):
                c = list(n)
                c[u] -= du
                c[v] -= dv
                return rank[c[2], c[1], c[0]]
            A, B, Cc, Dd = cell(1, 1), cell(0, 1), cell(0, 0), cell(1, 0)
            keys.append(3 * ((k * H + j) * W + i) + axis)
            quads.append((A, B, Cc, Dd) if lin else (A, Dd, Cc, B))
    tris = np.zeros((2 * len(quads), 3), dtype=np.uint32)
    for q, o in enumerate(np.argsort(keys, kind="stable")):
        v0, v1, v2, v3 = quads[o]
        assert min(v0, v1, v2, v3) >= 0, "a quad names a cell that is not active"
        tris[2 * q] = (v0, v1, v2)
        tris[2 * q + 1] = (v0, v2, v3)
    return verts, tris


# ---- OBJ --------------------------------------------------------------------------------------------------------------------------
def read_obj(path):
    """The ten-line parser of the tests: (positions [V, 3], normals [V, 3], faces [T, 3] 0-based position indices)."""
    v, vn, fc = [], [], []
    for line in open(path):
        w = line.split()
        if w and w[0] == "v":
            v.append([float(x) for x in w[1:4]])
        elif w and w[0] == "vn":
            vn.append([float(x) for x in w[1:4]])
        elif w and w[0] == "f":
            fc.append([int(x.split("/")[0]) - 1 for x in w[1:4]])
    return np.array(v, dtype=np.float64).reshape(-1, 3), np.array(vn, dtype=np.float64).reshape(-1, 3), np.array(fc, dtype=np.int64).reshape(-1, 3)
