"""3D surface extraction on the GPU: fs3_extract_surface / fs3_extract_surface_device against the checker of
tests/mesh3d_checker.cpp, byte for byte and with no exclusions: both arrays and both counts.  The checker is loaded with the state
downloaded from the SAME handle, so what is compared is the extractor alone, in both math modes; states are asserted finite first.
Particle counts are the sampler's: 16^3 (whole workgroups) and 18^3 (ragged); the node lattices are ragged against the 4 x 4 x 4
wave tile and the 256-node workgroup, and 49^3 has more than 256 workgroups, so the offset scan has real work."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.bitcmp import assert_identical
from tests.query3d_helpers import checker_of, make_sim
from tests.mesh3d_ref import Mesh3Checker

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f = np.float32
LATTICES = [(2, 2, 2), (5, 4, 3), (2, 65, 2), (65, 2, 2), (17, 9, 6), (33, 33, 33), (49, 49, 49)]
LARGE = [(33, 33, 33), (49, 49, 49)]


def raw_extract(fs, sim, dims, wmin, wmax, iso, vert_cap, tri_cap, sentinel=0xA5):
    """One blocking ABI call with the given capacities into sentinel-filled arrays one record longer: (verts, tris, (V, T))."""
    lib = fs.load_library()
    view = fs._abi.View3(fs.Vec3(*wmin), fs.Vec3(*wmax), *dims)
    verts = np.full((vert_cap + 1) * 40, sentinel, dtype=np.uint8)
    tris = np.full((tri_cap + 1) * 12, sentinel, dtype=np.uint8)
    counts = (C.c_uint32 * 2)()
    status = lib.fs3_extract_surface(sim._h, C.byref(view), float(iso), verts.ctypes.data if vert_cap else None, vert_cap,
                                     tris.ctypes.data if tri_cap else None, tri_cap, counts)
    assert status == fs._abi.FS_OK, lib.fs_last_error().decode()
    return verts, tris, (int(counts[0]), int(counts[1]))


def orientations(inside):
    """Interior crossing edges of a density mask [D, H, W] by the side of their low node: (low inside, low outside)."""
    from tests.mesh3d_ref import crossing_edges
    lows = np.concatenate([crossing_edges(inside, a)[1] for a in range(3)])
    return int(lows.sum()), int((~lows).sum())


# ---- 1. lattices and views -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ieee", "tolerance"])
@pytest.mark.parametrize("n", [16 ** 3, 18 ** 3])
def test_meshes_match_checker(fs, n, mode):
    from tests.mesh3d_ref import boundary_is_outside, directed_edges_balance, scene_views
    from tests.render3d_ref import iso_of
    mode = fs.FS_MATH_IEEE if mode == "ieee" else fs.FS_MATH_TOLERANCE
    sim, st, off, tick = make_sim(fs, n, mode)
    done = 0
    for steps in (1, 8, 60):
        while done < steps:
            sim.tick(tick)
            done += 1
        chk, p = checker_of(Mesh3Checker, sim, st, off, tick.mass)
        iso = iso_of(p)
        for name, (wmin, wmax) in scene_views(st, p).items():
            for dims in LATTICES:
                ctx = f"n {n} mode {mode} step {steps} view {name} lattice {dims}"
                want_v, want_t, want_c = chk.extract(dims, wmin, wmax, iso)
                got_v, got_t = sim.extract_surface(*dims, iso, wmin, wmax)
                assert (got_v.shape[0], got_t.shape[0]) == want_c, ctx
                assert_identical(got_v, want_v, ctx + " vertices")
                assert_identical(got_t, want_t, ctx + " triangles")
                if name == "outside":
                    assert want_c == (0, 0), ctx
                if dims in LARGE and name != "outside":
                    inside = chk.sample_grid(*dims, wmin, wmax)["density"] >= f(iso)
                    a, b = orientations(inside)
                    assert want_c[0] > 500 and a > 0 and b > 0 and 2 * (a + b) == want_c[1], ctx
                    if name == "overhang":
                        assert boundary_is_outside(inside) and directed_edges_balance(got_t), ctx
                    if name == "cut":
                        assert not directed_edges_balance(got_t), ctx
        chk.close()
    sim.close()


# ---- 2. dense cluster: long row ranges --------------------------------------------------------------------------------------------
def test_dense_cluster(fs):
    n = 12 ** 3
    st, off, tick = fs.dam_break_3d(n)
    sim = fs.FluidSimulation3D(st, device=0, initial_offset=off)
    rng = np.random.default_rng(23)
    h = st.smoothing_radius
    lo = np.float32([-st.size.x / 2 + 3 * h, -st.size.y / 2 + 2 * h, -st.size.z / 2 + 3 * h])     # a cell and its +x neighbour
    p = sim.download_particles()
    idx = rng.choice(n, 1400, replace=False)
    p["position"][idx] = (lo + rng.uniform(0.0, 1.0, size=(1400, 3)) * np.float32([2 * h, h, h])).astype(np.float32)
    p["predicted_position"] = p["position"]
    sim.upload_particles(p)
    sim.tick(tick)
    chk, q = checker_of(Mesh3Checker, sim, st, off, tick.mass)
    assert sim.sample(q["predicted_position"])["neighbours"].max() > 700
    c = lo.astype(np.float64) + [h, 0.5 * h, 0.5 * h]
    # a quarter of the cluster's central density: the few lattice particles left around it stay far below it
    iso = 0.25 * float(sim.sample(c[None, :].astype(np.float32))["density"][0])
    wmin, wmax = tuple(c - [3 * h, 2.5 * h, 2.5 * h]), tuple(c + [3 * h, 2.5 * h, 2.5 * h])
    dims = (25, 21, 21)                                   # spacing h / 4
    want_v, want_t, want_c = chk.extract(dims, wmin, wmax, iso)
    assert want_c[0] > 100 and want_c[1] > 100
    got_v, got_t = sim.extract_surface(*dims, iso, wmin, wmax)
    assert_identical(got_v, want_v, "cluster vertices")
    assert_identical(got_t, want_t, "cluster triangles")
    chk.close(); sim.close()


# ---- 3. tie to the public sampler (no checker) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ieee", "tolerance"])
def test_mesh_is_tied_to_the_public_sampler(fs, mode):
    from tests.mesh3d_ref import active_cells, scene_views
    from tests.render3d_ref import iso_of
    mode = fs.FS_MATH_IEEE if mode == "ieee" else fs.FS_MATH_TOLERANCE
    sim, st, off, tick = make_sim(fs, 18 ** 3, mode)
    for _ in range(8):
        sim.tick(tick)
    p = sim.download_particles()
    iso = iso_of(p)
    seen = 0
    for name, (wmin, wmax) in scene_views(st, p).items():
        for dims in ((17, 9, 6), (33, 33, 33)):
            verts, tris = sim.extract_surface(*dims, iso, wmin, wmax)
            inside = sim.sample_grid(*dims, world_min=wmin, world_max=wmax)["density"] >= f(iso)
            assert verts.shape[0] == int(active_cells(inside).sum()), (name, dims)
            a, b = orientations(inside)
            assert tris.shape[0] == 2 * (a + b), (name, dims)
            if not verts.shape[0]:
                continue
            seen += verts.shape[0]
            S = sim.sample(verts["position"])
            assert np.array_equal(S["density"].view(np.uint32), verts["density"].view(np.uint32)), name
            with np.errstate(all="ignore"):
                g = S["gradient"]
                gl = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(f)
                normal = np.where(gl[:, None] > 0, (-g) / gl[:, None], f(0)).astype(f)
                vel = np.where(S["weight"][:, None] > 0, S["velocity"] / S["weight"][:, None], f(0)).astype(f)
            assert np.array_equal(normal.view(np.uint32), verts["normal"].view(np.uint32)), name
            assert np.array_equal(vel.view(np.uint32), verts["velocity"].view(np.uint32)), name
    assert seen > 500
    sim.close()


# ---- 4. capacities ------------------------------------------------------------------------------------------------------------------
def test_capacities(fs):
    from tests.mesh3d_ref import scene_views
    from tests.render3d_ref import iso_of
    sim, st, off, tick = make_sim(fs, 18 ** 3, fs.FS_MATH_IEEE)
    for _ in range(8):
        sim.tick(tick)
    p = sim.download_particles()
    iso = iso_of(p)
    wmin, wmax = scene_views(st, p)["overhang"]
    dims = (33, 33, 33)
    full_v, full_t = sim.extract_surface(*dims, iso, wmin, wmax)
    V, T = full_v.shape[0], full_t.shape[0]
    assert V > 500 and T > 500
    for vc, tc in ((0, 0), (V - 1, T - 1), (1, 1), (V, T), (V + 3, 0), (0, T + 3), (1, T)):
        verts, tris, counts = raw_extract(fs, sim, dims, wmin, wmax, iso, vc, tc)
        assert counts == (V, T), (vc, tc)
        nv, nt = min(V, vc), min(T, tc)
        assert verts[:nv * 40].tobytes() == full_v[:nv].tobytes(), (vc, tc)
        assert tris[:nt * 12].tobytes() == full_t[:nt].tobytes(), (vc, tc)
        assert (verts[nv * 40:] == 0xA5).all() and (tris[nt * 12:] == 0xA5).all(), (vc, tc)
    sim.close()


# ---- 5. device form, stream-ordered between steps ---------------------------------------------------------------------------------
DEVICE_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r)
import torch                                   # torch FIRST: one HIP runtime per process
import numpy as np
import gpu_fluid_simulation_amd as g
from tests.mesh3d_ref import scene_views
from tests.render3d_ref import iso_of
from tests.track_ref import jitter_velocities
n = 18 ** 3
st, off, tick = g.dam_break_3d(n)
dev = torch.device("cuda", 0)
def make():
    sim = g.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.upload_particles(jitter_velocities(sim.download_particles(), 7))
    return sim
ref = make()
ref.tick(tick)
p0 = ref.download_particles()
iso = iso_of(p0)
wmin, wmax = scene_views(st, p0)["overhang"]
lattices = [(33, 33, 33), (17, 9, 6)]           # the second is smaller: the scratch of the first is reused
VC, TC = 6000, 700                              # room for every vertex, not for every triangle of the first
sim = make()
assert sim.stream_ptr
ext = torch.cuda.ExternalStream(sim.stream_ptr, device=dev)
bufs = []
with torch.cuda.stream(ext):
    for k in range(2):
        bufs.append((torch.full((VC * 10,), -1, dtype=torch.int32, device=dev), torch.full((TC * 3,), -1, dtype=torch.int32, device=dev),
                     torch.full((2,), -1, dtype=torch.int32, device=dev)))
    torch.cuda.synchronize()
    # step, extract, four steps, extract: no host synchronisation in between
    for k in range(2):
        for _ in range(1 if k == 0 else 4):
            sim.tick(tick)
        v, t, c = bufs[k]
        assert sim.extract_surface_device(*lattices[k], iso, v.data_ptr(), VC, t.data_ptr(), TC, c.data_ptr(), wmin, wmax) is None
sim.sync()
got = [(v.cpu().numpy(), t.cpu().numpy(), c.cpu().numpy()) for v, t, c in bufs]
for k in range(2):                             # re-run to each extracted step for the blocking form
    if k == 1:
        for _ in range(4):
            ref.tick(tick)
    want_v, want_t = ref.extract_surface(*lattices[k], iso, wmin, wmax)
    V, T = want_v.shape[0], want_t.shape[0]
    assert V > 20 and T > 20
    v, t, c = got[k]
    assert (int(c[0]), int(c[1])) == (V, T), "device counts of step %%d differ from the blocking form" %% (1 + 4 * k)
    nv, nt = min(V, VC), min(T, TC)
    assert v[:nv * 10].tobytes() == want_v[:nv].tobytes(), "device vertices of step %%d differ" %% (1 + 4 * k)
    assert t[:nt * 3].tobytes() == want_t[:nt].tobytes(), "device triangles of step %%d differ" %% (1 + 4 * k)
    assert (v[nv * 10:] == -1).all() and (t[nt * 3:] == -1).all(), "the device form wrote past its ranges"
assert got[0][2][0] <= VC and got[0][2][1] > TC, "the first extraction must overflow its triangle capacity only"
assert sim.download_particles().tobytes() == ref.download_particles().tobytes()
print("DEVICE_OK")
"""


def test_device_form_between_steps(fs):
    out = subprocess.run([sys.executable, "-c", DEVICE_SCRIPT % {"root": ROOT}], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "DEVICE_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 6. checks, in the order of the header -------------------------------------------------------------------------------------------
def test_checks_in_the_headers_order_and_state_guards(fs):
    lib = fs.load_library()
    inv, ok = fs._abi.FS_ERR_INVALID, fs._abi.FS_OK
    sim, st, off, tick = make_sim(fs, 16 ** 3, fs.FS_MATH_IEEE)          # created and uploaded to: no step yet
    h = sim._h
    verts = np.zeros(4, dtype=fs.MESH_VERTEX_DTYPE)
    tris = np.zeros((4, 3), dtype=np.uint32)
    counts = np.full(2, 77, dtype=np.uint32)
    Vp, Tp, Cp = verts.ctypes.data, tris.ctypes.data, counts.ctypes.data
    err = lambda: lib.fs_last_error().decode()                                                   # noqa: E731
    calls = (lib.fs3_extract_surface, lib.fs3_extract_surface_device)    # the device form is refused before a pointer is touched
    nan, inf = float("nan"), float("inf")

    def view(w=5, hh=4, d=3):
        return fs._abi.View3(fs.Vec3(-1, -1, -1), fs.Vec3(1, 1, 1), w, hh, d)

    good = view()
    bad_views = [view(w=1), view(hh=1), view(d=1), view(w=0), view(w=1 << 13, hh=1 << 13, d=2), view(w=0xFFFFFFFF, hh=0xFFFFFFFF, d=0xFFFFFFFF),
                 view(w=(1 << 13) + 1, hh=1 << 13, d=1)]
    bad_isos = [0.0, -1.0, nan, inf, -inf]

    def refused(call, v, iso, vp, vc, tp, tc, cp, text):
        status = call(h, C.byref(v) if v is not None else None, iso, vp, vc, tp, tc, cp)
        assert status == inv and text in err(), (status, err(), text)

    def all_before_the_state_check():
        for call in calls:
            # 1. NULL handle (before anything else), view, counts
            assert call(None, C.byref(bad_views[0]), nan, None, 1, None, 1, None) == inv and "null" in err()
            refused(call, None, 1.0, Vp, 4, Tp, 4, Cp, "null argument")
            refused(call, good, 1.0, Vp, 4, Tp, 4, None, "null argument")
            refused(call, bad_views[0], nan, None, 1, None, 1, None, "null argument")
            # 2. the lattice, before iso
            for v in bad_views:
                refused(call, v, nan, None, 1, None, 1, Cp, "lattice size")
            # 3. iso, before the arrays
            for iso in bad_isos:
                refused(call, good, iso, None, 1, None, 1, Cp, "iso")
            # 4. a NULL array with a capacity
            refused(call, good, 1.0, None, 1, Tp, 4, Cp, "null array")
            refused(call, good, 1.0, Vp, 4, None, 1, Cp, "null array")

    def stale():
        for call in calls:
            refused(call, good, 1.0, Vp, 4, Tp, 4, Cp, "needs a step")
            refused(call, good, 1.0, None, 0, None, 0, Cp, "needs a step")
            refused(call, good, 1.0, None, 1, Tp, 4, Cp, "null array")       # 4 before 5

    def valid():
        assert lib.fs3_extract_surface(h, C.byref(good), 1.0, Vp, 4, Tp, 4, Cp) == ok
        assert lib.fs3_extract_surface(h, C.byref(good), 1.0, None, 0, None, 0, Cp) == ok
        assert lib.fs3_extract_surface(h, C.byref(view(2, 2, 2)), 1e30, None, 0, Tp, 4, Cp) == ok and (counts == 0).all()
        assert lib.fs3_extract_surface(h, C.byref(view(1 << 13, 1 << 12, 2)), 1e30, Vp, 4, None, 0, Cp) == ok and (counts == 0).all()   # 2^26 nodes

    all_before_the_state_check()
    stale()                                          # 5. before the first step
    assert not verts.view(np.uint8).any() and not tris.any() and (counts == 77).all()
    sim.tick(tick)
    valid()
    all_before_the_state_check()
    sim.upload_particles(sim.download_particles()[:0])      # an upload of nothing changes nothing
    valid()
    sim.upload_particles(sim.download_particles()[:10])     # a partial upload counts
    stale()
    sim.tick(tick)
    valid()
    sim.close()


# ---- 7. extraction leaves the state alone --------------------------------------------------------------------------------------------
def test_extraction_leaves_the_state_alone(fs):
    from tests.render3d_ref import iso_of
    a, st, off, tick = make_sim(fs, 18 ** 3, fs.FS_MATH_IEEE)
    b, _, _, _ = make_sim(fs, 18 ** 3, fs.FS_MATH_IEEE)
    iso = None
    for s in range(20):
        a.tick(tick); b.tick(tick)
        if s % 3 == 0:
            iso = iso or iso_of(a.download_particles())
            verts, tris = a.extract_surface(33 - s, 25, 17 + s, iso)
            assert verts.shape[0] > 20 and tris.shape[0] > 20
    assert a.download_particles().tobytes() == b.download_particles().tobytes()
    a.close(); b.close()
