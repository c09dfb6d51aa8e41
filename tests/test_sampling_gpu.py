"""GPU tests of field sampling: k_sample against the CPU checker (tests/sample_checker.cpp on the unchanged
oracle's cell walk), byte for byte.  For every case the records, start indices, uniform (and channels) are downloaded from the
GPU handle and loaded into the checker, so the comparison is about the sampler alone, on whatever state the handle's sort and
math mode produced.  No comparison masks anything: the states are asserted finite first."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPSILON_F = np.float32(1.19209290e-07)


def make_sim(fs, n, seed=7, quirks=True, counting=False, **kw):
    from tests.track_ref import jitter_velocities
    st, off, tick = fs.dam_break_2d(n)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, ref_quirks=quirks,
                             sort_mode=fs.FS_SORT_COUNTING if counting else fs.FS_SORT_BITONIC, **kw)
    sim.upload_particles(jitter_velocities(sim.download_particles(), seed))
    return sim, st, off, tick


def load_checker(fs, sim, st, off, quirks=True):
    """-> (checker holding the handle's downloaded state, the records, the channels or None)."""
    from tests.sample_ref import SampleChecker, set_threads
    set_threads(16)
    chk = SampleChecker(st, off, ref_quirks=quirks)
    p = sim.download_particles()
    for f in ("position", "predicted_position", "velocity", "density"):
        assert np.isfinite(p[f]).all(), f"non-finite {f}: share masked must be 0"
    chk.load(p, sim.download_start_indices(), sim.uniform())
    ch = sim.track_channels
    attr = np.stack([sim.attribute(c) for c in range(ch)]) if ch > 0 else None
    return chk, p, attr


def assert_samples_equal(sim, chk, pts, attr, ctx):
    if attr is not None:
        got, ga = sim.sample(pts, attributes=True)
    else:
        got, ga = sim.sample(pts), None
    want, wa = chk.sample(pts, attr)
    if got.tobytes() != want.tobytes():
        bad = [f for f in want.dtype.names if np.ascontiguousarray(got[f]).tobytes() != np.ascontiguousarray(want[f]).tobytes()]
        k = int(np.flatnonzero((got.view(np.uint8).reshape(-1, 24) != want.view(np.uint8).reshape(-1, 24)).any(axis=1))[0])
        raise AssertionError(f"{ctx}: fs_sample differs in fields {bad}; first at query {k}: got {got[k]}, want {want[k]}")
    if attr is not None:
        assert ga.shape == wa.shape and ga.tobytes() == wa.tobytes(), f"{ctx}: channel sums differ"
    return got


def query_sets(st, p, rng):
    """name -> points: own positions (slot order), the same shuffled, uniform over 1.2 x the domain, points exactly on cell
    boundaries and on the domain's corners."""
    sx, sy, h = float(st.size.x), float(st.size.y), np.float32(st.smoothing_radius)
    own = np.ascontiguousarray(p["predicted_position"])
    m = 4000
    uni = np.stack([rng.uniform(-0.6 * sx, 0.6 * sx, m), rng.uniform(-0.6 * sy, 0.6 * sy, m)], axis=1).astype(np.float32)
    f = np.float32
    bx = (np.arange(0, 40, dtype=f) * h - f(sx) * f(0.5)).astype(f)          # x + bounds/2 is a multiple of h (up to rounding)
    by = (np.arange(0, 40, dtype=f) * h - f(sy) * f(0.5)).astype(f)
    edges = np.stack(np.meshgrid(bx, by), axis=-1).reshape(-1, 2)
    low = own[np.argsort(own[:, 1])[-200:]]                                    # ... and boundaries next to particles
    snap = low.copy()
    snap[:, 0] = (np.floor((low[:, 0] + f(sx) * f(0.5)) / h) * h - f(sx) * f(0.5)).astype(f)
    corners = np.array([[-sx / 2, -sy / 2], [sx / 2, -sy / 2], [-sx / 2, sy / 2], [sx / 2, sy / 2], [0.0, sy / 2], [0.0, -sy / 2]], dtype=f)
    return {"own": own, "shuffled": own[rng.permutation(own.shape[0])], "uniform": uni,
            "boundaries": np.concatenate([edges, snap, corners]).astype(f)}


def check_all_sets(fs, sim, st, off, quirks, ieee, ctx, sizes=()):
    chk, p, attr = load_checker(fs, sim, st, off, quirks)
    rng = np.random.default_rng(5)
    sets = query_sets(st, p, rng)
    for name, pts in sets.items():
        got = assert_samples_equal(sim, chk, pts, attr, f"{ctx} {name}")
        if name == "own":
            assert np.array_equal(got["cell"], p["grid"])
            if ieee:        # the known answer that ties the sampler to the step
                d = np.maximum(np.maximum(got["density"], EPSILON_F), np.float32(0.1))
                assert np.array_equal(d.view(np.uint32), p["density"].view(np.uint32)), f"{ctx}: density identity"
        if name == "uniform":
            assert got["neighbours"].any() and not got["neighbours"].all(), "the random set must hit the fluid and miss it"
    for m in sizes:
        assert_samples_equal(sim, chk, sets["shuffled"][:m], attr, f"{ctx} n={m}")
    chk.close()


# ---- 1. small scenes: both sorts, both quirk settings, after 1, 8 and 260 steps ------------------------------------------
@pytest.mark.parametrize("quirks", [True, False])
@pytest.mark.parametrize("counting", [False, True])
@pytest.mark.parametrize("n", [4096, 5000])
def test_sampler_matches_checker_small(fs, n, counting, quirks):
    sim, st, off, tick = make_sim(fs, n, quirks=quirks, counting=counting)
    done = 0
    for steps in (1, 8, 260):
        while done < steps:
            sim.tick(tick)
            done += 1
        check_all_sets(fs, sim, st, off, quirks, True, f"n={n} counting={counting} quirks={quirks} steps={steps}",
                       sizes=(1, 63, 64, 65, 257) if steps == 8 else ())
    sim.close()


# ---- 2. every math mode: the sampler is exact on whatever state the mode produced ---------------------------------------
@pytest.mark.parametrize("mode", ["FS_MATH_IEEE", "FS_MATH_WGSL_ULP", "FS_MATH_TOLERANCE"])
@pytest.mark.parametrize("n,counting", [(5000, False), (65536, False), (65536, True)])
def test_sampler_is_exact_in_every_math_mode(fs, n, counting, mode):
    sim, st, off, tick = make_sim(fs, n, counting=counting, math_mode=getattr(fs, mode))
    for _ in range(8):
        sim.tick(tick)
    check_all_sets(fs, sim, st, off, True, mode == "FS_MATH_IEEE", f"n={n} counting={counting} {mode}")
    sim.close()


@pytest.mark.parametrize("mode", ["FS_MATH_IEEE", "FS_MATH_TOLERANCE"])
def test_mass_other_than_one(fs, mode):
    """m / rho_j by the division (the reciprocal the density pass keeps serves m == 1.0f only)."""
    sim, st, off, tick = make_sim(fs, 5000, math_mode=getattr(fs, mode))
    tick.mass = 1.5
    for _ in range(8):
        sim.tick(tick)
    check_all_sets(fs, sim, st, off, True, mode == "FS_MATH_IEEE", f"mass 1.5 {mode}")
    sim.close()


def test_one_million_particles(fs):
    sim, st, off, tick = make_sim(fs, 1_000_000)
    for _ in range(3):
        sim.tick(tick)
    check_all_sets(fs, sim, st, off, True, True, "n=1M")
    sim.close()


def test_with_surface_tension_on(fs):
    sim, st, off, tick = make_sim(fs, 5000, surface_tension=True)
    tick.surface_tension_coefficient = 0.05
    for _ in range(8):
        sim.tick(tick)
    assert sim.surface_tension_forces().any()
    check_all_sets(fs, sim, st, off, True, True, "surface tension on")
    sim.close()


# ---- 3. channels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counting", [False, True])
@pytest.mark.parametrize("channels", [0, 2, 4])
def test_channels(fs, channels, counting):
    n = 5000
    sim, st, off, tick = make_sim(fs, n, counting=counting, track=channels)
    rng = np.random.default_rng(17)
    for c in range(channels):
        v = rng.uniform(-3.0, 3.0, n).astype(np.float32)
        v[rng.integers(0, n, n // 4)] = 0.0
        v[rng.integers(0, n, n // 8)] = -0.0
        if c == 1:
            v[:] = -0.0                       # a channel of negative zeros: its sums are -0 terms only
        sim.set_attribute(c, v)
    for _ in range(8):
        sim.tick(tick)
    if channels == 0:
        with pytest.raises(fs.FluidSimError) as e:
            sim.sample(np.zeros((3, 2), dtype=np.float32), attributes=True)
        assert e.value.status == fs._abi.FS_ERR_INVALID
        buf = np.zeros(8, dtype=np.float32)
        out = np.zeros(2, dtype=fs.SAMPLE_DTYPE)
        assert fs.load_library().fs_sample_points(sim._h, buf.ctypes.data_as(C.c_void_p), 2, out.ctypes.data_as(C.c_void_p),
                                                  buf.ctypes.data_as(C.c_void_p)) == fs._abi.FS_ERR_INVALID
    check_all_sets(fs, sim, st, off, True, True, f"C={channels} counting={counting}", sizes=(1, 65))
    if channels:
        p = sim.download_particles()
        got, ga = sim.sample(p["predicted_position"], attributes=True, normalise=True)
        assert ga.shape == (channels, n) and np.isfinite(ga).all()
        assert not ga[1].any(), "Shepard value of an all-zero channel"
    sim.close()


# ---- 4. rows longer than any tile or fast path --------------------------------------------------------------------------------
@pytest.mark.parametrize("counting", [False, True])
def test_dense_cluster(fs, counting):
    """3000 of 4096 particles uploaded into one cell and its neighbour (rows of ~3000 candidates), then one step."""
    n = 4096
    st, off, tick = fs.dam_break_2d(n)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off, sort_mode=fs.FS_SORT_COUNTING if counting else fs.FS_SORT_BITONIC, track=2)
    rng = np.random.default_rng(23)
    p = sim.download_particles()
    c = np.array([0.31, 0.17], dtype=np.float32)
    p["position"][:3000] = c + rng.uniform(-0.15, 0.15, (3000, 2)).astype(np.float32)
    p["predicted_position"] = p["position"]
    sim.upload_particles(p)
    for ch in range(2):
        sim.set_attribute(ch, rng.uniform(-1.0, 1.0, n).astype(np.float32))
    sim.tick(tick)
    chk, q, attr = load_checker(fs, sim, st, off)
    assert np.bincount(q["grid"]).max() > 700, "the cluster must exceed a 640-entry tile"
    near = (c + rng.uniform(-0.5, 0.5, (1000, 2))).astype(np.float32)
    for name, pts in (("own", q["predicted_position"]), ("near", near)):
        got = assert_samples_equal(sim, chk, np.ascontiguousarray(pts), attr, f"cluster {name}")
    assert got["neighbours"].max() > 700
    chk.close(); sim.close()


# ---- 5. the grid form is the point form on the pixel centres --------------------------------------------------------------
@pytest.mark.parametrize("counting", [False, True])
def test_grid_equals_points(fs, counting):
    from tests.sample_ref import grid_points
    n = 65536
    sim, st, off, tick = make_sim(fs, n, counting=counting, track=3)
    rng = np.random.default_rng(4)
    for c in range(3):
        sim.set_attribute(c, rng.uniform(-1.0, 1.0, n).astype(np.float32))
    for _ in range(8):
        sim.tick(tick)
    chk, _, attr = load_checker(fs, sim, st, off)
    sx, sy = float(st.size.x), float(st.size.y)
    views = [(64, 48, None, None),                                           # the domain (render_density's default view)
             (101, 37, (-sx / 4, -sy / 8), (sx / 3, sy / 2)),                # inside, non-square, 3737 pixels
             (50, 77, (-sx, -sy), (sx, sy)),                                 # larger than the domain
             (1, 300, (-sx / 2, -sy / 2), (sx / 2, sy / 2)), (17, 1, (-1.0, 0.0), (1.0, sy / 2))]
    hit = 0
    for (w, h, wmin, wmax) in views:
        g, ga = sim.sample_grid(w, h, wmin, wmax, attributes=True)
        wmin = wmin if wmin is not None else (-sx / 2, -sy / 2)
        wmax = wmax if wmax is not None else (sx / 2, sy / 2)
        pts = grid_points(w, h, wmin, wmax)
        q, qa = sim.sample(pts, attributes=True)
        assert g.shape == (h, w) and ga.shape == (3, h, w)
        assert g.tobytes() == q.tobytes() and ga.tobytes() == qa.tobytes(), f"grid {w}x{h} != points"
        want, wa = chk.sample_grid(w, h, wmin, wmax, attr)
        assert g.tobytes() == want.tobytes() and ga.tobytes() == wa.tobytes(), f"grid {w}x{h} != checker"
        hit += int(g["neighbours"].any())
    assert hit >= 4
    chk.close(); sim.close()


# ---- 6. device pointers, stream-ordered between steps -------------------------------------------------------------------------
DEVICE_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r)
import torch                                   # torch FIRST: one HIP runtime per process
import numpy as np
import gpu_fluid_simulation_amd as g
from tests.sample_ref import SampleChecker, set_threads
from tests.track_ref import jitter_velocities
set_threads(16)
n, m, C = 65536, 50000, 2
st, off, tick = g.dam_break_2d(n)
dev = torch.device("cuda", 0)
rng = np.random.default_rng(2)
sx, sy = float(st.size.x), float(st.size.y)
pts = np.stack([rng.uniform(-0.6 * sx, 0.6 * sx, m), rng.uniform(-0.2 * sy, 0.6 * sy, m)], axis=1).astype(np.float32)
ch = [rng.uniform(-1.0, 1.0, n).astype(np.float32) for _ in range(C)]
def make():
    sim = g.FluidSimulation(st, device=0, initial_offset=off, track=C)
    sim.upload_particles(jitter_velocities(sim.download_particles(), 7))
    for c in range(C):
        sim.set_attribute(c, ch[c])
    return sim
sim = make()
ext = torch.cuda.ExternalStream(sim.stream_ptr, device=dev)
outs, attrs = [], []
with torch.cuda.stream(ext):
    d_pts = torch.from_numpy(pts).to(dev, non_blocking=False)
    for k in range(2):
        outs.append(torch.zeros(m * 6, dtype=torch.int32, device=dev))
        attrs.append(torch.zeros(C * m, dtype=torch.float32, device=dev))
    torch.cuda.synchronize()
    # step, sample, step, sample: no host synchronisation in between
    for k in range(2):
        for _ in range(4):
            sim.tick(tick)
        sim.sample_device(d_pts.data_ptr(), m, outs[k].data_ptr(), attrs[k].data_ptr())
sim.sync()
got = [(o.cpu().numpy().tobytes(), a.cpu().numpy().tobytes()) for o, a in zip(outs, attrs)]
ref = make()                                   # re-run to each sampled step for the download
for k in range(2):
    for _ in range(4):
        ref.tick(tick)
    chk = SampleChecker(st, off)
    chk.load(ref.download_particles(), ref.download_start_indices(), ref.uniform())
    attr = np.stack([ref.attribute(c) for c in range(C)])
    want, wa = chk.sample(pts, attr)
    assert want["neighbours"].any()
    assert got[k][0] == want.tobytes(), "device samples of step %%d differ" %% (4 * (k + 1))
    assert got[k][1] == wa.tobytes(), "device channel sums of step %%d differ" %% (4 * (k + 1))
    chk.close()
assert got[0][0] != got[1][0], "the two sampled states must differ"
assert sim.download_particles().tobytes() == ref.download_particles().tobytes()
print("DEVICE_OK")
"""


def test_device_pointers_between_steps(fs):
    out = subprocess.run([sys.executable, "-c", DEVICE_SCRIPT % {"root": ROOT}], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "DEVICE_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 7. error paths ------------------------------------------------------------------------------------------------------------
def test_error_paths(fs):
    lib = fs.load_library()
    inv, uns = fs._abi.FS_ERR_INVALID, fs._abi.FS_ERR_UNSUPPORTED
    sim, st, off, tick = make_sim(fs, 4096)
    pts = np.zeros((4, 2), dtype=np.float32)
    out = np.zeros(4, dtype=fs.SAMPLE_DTYPE)
    P, O = pts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    view = fs._abi.View(fs.Vec2(-1.0, -1.0), fs.Vec2(1.0, 1.0), 2, 2)
    assert lib.fs_sample_points(sim._h, P, 4, O, None) == inv                       # before the first step
    assert lib.fs_sample_grid(sim._h, C.byref(view), O, None) == inv
    assert lib.fs_sample_points_device(sim._h, P, 4, O, None) == inv               # (checked before anything is enqueued)
    assert lib.fs_sample_points(sim._h, P, 0, O, None) == fs._abi.FS_OK            # n == 0 touches nothing
    sim.tick(tick)
    assert lib.fs_sample_points(sim._h, P, 4, O, None) == fs._abi.FS_OK
    assert lib.fs_sample_points(sim._h, None, 4, O, None) == inv
    assert lib.fs_sample_points(sim._h, P, 4, None, None) == inv
    assert lib.fs_sample_points(sim._h, P, (1 << 28) + 1, O, None) == inv
    assert lib.fs_sample_points(sim._h, P, 4, O, P) == inv                          # attr_out without tracking
    assert lib.fs_sample_grid(sim._h, None, O, None) == inv
    for w, h in ((0, 2), (2, 0), (1 << 15, 1 << 14)):
        bad = fs._abi.View(fs.Vec2(-1.0, -1.0), fs.Vec2(1.0, 1.0), w, h)
        assert lib.fs_sample_grid(sim._h, C.byref(bad), O, None) == inv
    p = sim.download_particles()
    sim.upload_particles(p)                                                         # between an upload and the next step
    with pytest.raises(fs.FluidSimError) as e:
        sim.sample(pts)
    assert e.value.status == inv
    sim.tick(tick)
    sim.sample(pts)
    sim.upload_start_indices(sim.download_start_indices())
    assert lib.fs_sample_grid(sim._h, C.byref(view), O, None) == inv
    sim.tick(tick)
    assert sim.sample_grid(2, 2).shape == (2, 2)
    sim.close()
    st2, _, _ = fs.dam_break_2d(16384)
    slab = fs.SlabSimulation(st2, 10, 40, False, False, 16384 + 2 * 2048, 2048, 66, device=0)
    assert lib.fs_sample_points(slab._h, P, 4, O, None) == uns
    assert lib.fs_sample_points_device(slab._h, P, 4, O, None) == uns
    assert lib.fs_sample_grid(slab._h, C.byref(view), O, None) == uns
    slab.close()


# ---- 8. sampling changes no bit of the simulation ---------------------------------------------------------------------------
@pytest.mark.parametrize("counting", [False, True])
def test_sampling_leaves_the_state_alone(fs, counting):
    n = 5000
    a, st, off, tick = make_sim(fs, n, counting=counting, track=1)
    b, _, _, _ = make_sim(fs, n, counting=counting, track=1)
    rng = np.random.default_rng(9)
    pts = rng.uniform(-5.0, 5.0, (777, 2)).astype(np.float32)
    for s in range(20):
        a.tick(tick); b.tick(tick)
        if s % 3 == 0:
            a.sample(pts, attributes=True)
        if s % 5 == 0:
            a.sample_grid(33, 19)
    assert a.download_particles().tobytes() == b.download_particles().tobytes()
    assert a.download_start_indices().tobytes() == b.download_start_indices().tobytes()
    assert a.particle_ids().tobytes() == b.particle_ids().tobytes()
    a.close(); b.close()
