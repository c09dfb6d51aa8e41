"""3D field sampling on the GPU: fs3_sample_points / fs3_sample_points_device / fs3_sample_grid against the
checker of tests/sample3d_checker.cpp, byte for byte.  The checker is loaded with the state downloaded from the SAME handle,
so what is compared is the sampler alone, in both math modes; states are asserted finite first, so that no comparison masks
anything.  Sizes are the smallest at which the kernel can go wrong: 16^3 = 4096 (whole workgroups), 18^3 = 5832 (ragged
against the workgroup and the wave), 33^3 (ragged everything) once."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.bitcmp import assert_identical
from tests.query3d_helpers import checker_of, make_sim
from tests.sample3d_ref import Sample3Checker

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPSILON_F = np.float32(1.19209290e-07)
f = np.float32


def check_query_sets(fs, sim, st, off, tick, mode, ctx):
    from tests.sample3d_ref import boundary_points, uniform_points
    chk, p = checker_of(Sample3Checker, sim, st, off, tick.mass)
    own = p["predicted_position"].copy()
    out = sim.sample(own)
    assert_identical(out, chk.sample(own), f"{ctx}: own positions")
    assert np.array_equal(out["cell"], p["grid"]), ctx
    assert (out["neighbours"] >= 1).all(), ctx
    if mode == fs.FS_MATH_IEEE:
        got = np.maximum(np.maximum(out["density"], EPSILON_F), f(0.1))
        assert np.array_equal(got.view(np.uint32), p["density"].view(np.uint32)), f"{ctx}: density identity"
    rng = np.random.default_rng(1)
    shuffled = own[rng.permutation(own.shape[0])]
    assert_identical(sim.sample(shuffled), chk.sample(shuffled), f"{ctx}: shuffled")
    uni = uniform_points(st, 4000, seed=2)
    out = sim.sample(uni)
    assert (out["neighbours"] > 0).sum() > 100 and (out["neighbours"] == 0).sum() > 100, ctx
    assert_identical(out, chk.sample(uni), f"{ctx}: uniform")
    bnd = boundary_points(st, p, 300, seed=3)
    assert_identical(sim.sample(bnd), chk.sample(bnd), f"{ctx}: boundary")
    for m in (1, 63, 64, 65, 257):
        assert_identical(sim.sample(own[100:100 + m]), chk.sample(own[100:100 + m]), f"{ctx}: {m} queries")
    chk.close()


# ---- 1. query sets ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ieee", "tolerance"])
@pytest.mark.parametrize("n", [16 ** 3, 18 ** 3])
def test_query_sets_match_checker(fs, n, mode):
    mode = fs.FS_MATH_IEEE if mode == "ieee" else fs.FS_MATH_TOLERANCE
    sim, st, off, tick = make_sim(fs, n, mode)
    done = 0
    for steps in (1, 8, 60):
        while done < steps:
            sim.tick(tick)
            done += 1
        check_query_sets(fs, sim, st, off, tick, mode, f"n {n} mode {mode} step {steps}")
    sim.close()


def test_ragged_everything_once(fs):
    sim, st, off, tick = make_sim(fs, 33 ** 3, fs.FS_MATH_IEEE)
    for _ in range(3):
        sim.tick(tick)
    check_query_sets(fs, sim, st, off, tick, fs.FS_MATH_IEEE, "n 33^3 step 3")
    sim.close()


# ---- 2. mass ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ieee", "tolerance"])
def test_mass_other_than_one(fs, mode):
    mode = fs.FS_MATH_IEEE if mode == "ieee" else fs.FS_MATH_TOLERANCE
    sim, st, off, tick = make_sim(fs, 18 ** 3, mode)
    heavy = fs.TickSettings3.from_buffer_copy(tick)
    heavy.mass = 1.5
    for _ in range(5):
        sim.tick(heavy)
    check_query_sets(fs, sim, st, off, heavy, mode, f"mass 1.5 mode {mode}")
    sim.tick(tick)                                  # the mass of the LAST step is what counts
    check_query_sets(fs, sim, st, off, tick, mode, f"mass back to 1 mode {mode}")
    sim.close()


# ---- 3. dense cluster ---------------------------------------------------------------------------------------------------------
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
    chk, q = checker_of(Sample3Checker, sim, st, off, tick.mass)
    own = q["predicted_position"].copy()
    out = sim.sample(own)
    assert out["neighbours"].max() > 700
    assert_identical(out, chk.sample(own), "cluster: own positions")
    near = (lo + rng.uniform(-0.5, 1.5, size=(1000, 3)) * np.float32([2 * h, h, h])).astype(np.float32)
    out = sim.sample(near)
    assert out["neighbours"].max() > 700
    assert_identical(out, chk.sample(near), "cluster: nearby points")
    chk.close(); sim.close()


# ---- 4. grid == points == checker ---------------------------------------------------------------------------------------------
def test_grid_equals_points_equals_checker(fs):
    from tests.sample3d_ref import grid_points
    sim, st, off, tick = make_sim(fs, 16 ** 3, fs.FS_MATH_IEEE)
    for _ in range(8):
        sim.tick(tick)
    chk, p = checker_of(Sample3Checker, sim, st, off, tick.mass)
    sx, sy, sz = st.size.x, st.size.y, st.size.z
    c = p["predicted_position"].mean(axis=0)
    dom = ((-sx / 2, -sy / 2, -sz / 2), (sx / 2, sy / 2, sz / 2))
    views = [(16, 12, 9) + dom,
             (21, 7, 5, (c[0] - 0.9, c[1] - 0.35, c[2] - 0.6), (c[0] + 0.4, c[1] + 0.3, c[2] + 0.5)),        # a non-cubic sub-box
             (10, 9, 11, (-0.7 * sx, -0.7 * sy, -0.7 * sz), (0.7 * sx, 0.7 * sy, 0.7 * sz)),               # larger than the domain
             (33, 17, 1, (-sx / 2, -sy / 2, c[2]), (sx / 2, sy / 2, c[2])),                                 # a slice through the fluid
             (1, 1, 40, (c[0], c[1], -sz / 2), (c[0], c[1], sz / 2))]                                       # a line
    assert sim.sample_grid(4, 3).shape == (1, 3, 4)
    assert_identical(sim.sample_grid(16, 12, 9), sim.sample_grid(*views[0]), "default view = the whole domain")
    hit = 0
    for w, h, d, wmin, wmax in views:
        got = sim.sample_grid(w, h, d, wmin, wmax)
        assert got.shape == (d, h, w)
        pts = grid_points(w, h, d, wmin, wmax)
        assert_identical(got.ravel(), sim.sample(pts), f"grid {w}x{h}x{d} against the point form")
        assert_identical(got, chk.sample_grid(w, h, d, wmin, wmax), f"grid {w}x{h}x{d} against the checker")
        if d == 1:
            assert wmin[2] == wmax[2] and (pts[:, 2] == f(wmin[2])).all()
        hit += int((got["neighbours"] > 0).any())
    assert hit >= 4
    chk.close(); sim.close()


# ---- 5. device pointers, stream-ordered between steps -------------------------------------------------------------------------
DEVICE_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r)
import torch                                   # torch FIRST: one HIP runtime per process
import numpy as np
import gpu_fluid_simulation_amd as g
from tests.sample3d_ref import Sample3Checker, uniform_points
from tests.track_ref import jitter_velocities
n, m = 18 ** 3, 3001
st, off, tick = g.dam_break_3d(n)
dev = torch.device("cuda", 0)
pts = uniform_points(st, m, seed=9, scale=1.0)
def make():
    sim = g.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.upload_particles(jitter_velocities(sim.download_particles(), 7))
    return sim
sim = make()
assert sim.stream_ptr
ext = torch.cuda.ExternalStream(sim.stream_ptr, device=dev)
outs = []
with torch.cuda.stream(ext):
    d_pts = torch.from_numpy(pts).to(dev, non_blocking=False)
    for k in range(2):
        outs.append(torch.zeros(m * 10, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    # step, sample, step, sample: no host synchronisation in between
    for k in range(2):
        for _ in range(4):
            sim.tick(tick)
        sim.sample_device(d_pts.data_ptr(), m, outs[k].data_ptr())
sim.sync()
got = [o.cpu().numpy().tobytes() for o in outs]
ref = make()                                   # re-run to each sampled step for the download
for k in range(2):
    for _ in range(4):
        ref.tick(tick)
    p = ref.download_particles()
    assert np.isfinite(p["predicted_position"]).all() and np.isfinite(p["velocity"]).all() and np.isfinite(p["density"]).all()
    chk = Sample3Checker(st, off).load(p, tick.mass)
    want = chk.sample(pts)
    assert want["neighbours"].any()
    assert got[k] == want.tobytes(), "device samples of step %%d differ" %% (4 * (k + 1))
    chk.close()
assert got[0] != got[1], "the two sampled states must differ"
assert sim.download_particles().tobytes() == ref.download_particles().tobytes()
print("DEVICE_OK")
"""


def test_device_pointers_between_steps(fs):
    out = subprocess.run([sys.executable, "-c", DEVICE_SCRIPT % {"root": ROOT}], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "DEVICE_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 6. error paths, in the order of the header -----------------------------------------------------------------------------------
def test_error_paths(fs):
    lib = fs.load_library()
    inv, ok = fs._abi.FS_ERR_INVALID, fs._abi.FS_OK
    sim, st, off, tick = make_sim(fs, 16 ** 3, fs.FS_MATH_IEEE)          # created and uploaded to: no step yet
    h = sim._h
    pts = np.zeros((8, 3), dtype=np.float32)
    out = np.zeros(8, dtype=fs.SAMPLE3_DTYPE)
    P, O = pts.ctypes.data, out.ctypes.data
    view = lambda w, hh, d: fs._abi.View3(fs.Vec3(-1, -1, -1), fs.Vec3(1, 1, 1), w, hh, d)      # noqa: E731
    err = lambda: lib.fs_last_error().decode()                                                   # noqa: E731

    def refused(status, text):
        assert status == inv and text in err(), (status, err())

    def all_before_the_state_check():
        # 1. NULL handle
        refused(lib.fs3_sample_points(None, P, 8, O), "null")
        refused(lib.fs3_sample_points_device(None, P, 8, O), "null")
        refused(lib.fs3_sample_grid(None, C.byref(view(2, 2, 2)), O), "null")
        # 2. grid form: NULL view, a zero extent, more than 2^28 voxels (the out pointer is never reached)
        refused(lib.fs3_sample_grid(h, None, O), "null")
        for w, hh, d in ((0, 2, 2), (2, 0, 2), (2, 2, 0), (1 << 14, 1 << 14, 2), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)):
            refused(lib.fs3_sample_grid(h, C.byref(view(w, hh, d)), None), "grid size")
        # 3. n == 0: FS_OK, nothing touched
        assert lib.fs3_sample_points(h, None, 0, None) == ok
        assert lib.fs3_sample_points_device(h, None, 0, None) == ok
        # 4. NULL points / out
        refused(lib.fs3_sample_points(h, None, 8, O), "null")
        refused(lib.fs3_sample_points(h, P, 8, None), "null")
        refused(lib.fs3_sample_points_device(h, None, 8, O), "null")
        refused(lib.fs3_sample_points_device(h, P, 8, None), "null")
        refused(lib.fs3_sample_grid(h, C.byref(view(2, 2, 2)), None), "null")
        # 5. n > 2^28
        refused(lib.fs3_sample_points(h, P, (1 << 28) + 1, O), "2^28")
        refused(lib.fs3_sample_points_device(h, P, (1 << 28) + 1, O), "2^28")

    def stale():
        refused(lib.fs3_sample_points(h, P, 8, O), "needs a step")
        refused(lib.fs3_sample_points_device(h, P, 8, O), "needs a step")
        refused(lib.fs3_sample_grid(h, C.byref(view(2, 2, 2)), O), "needs a step")

    def valid():
        assert lib.fs3_sample_points(h, P, 8, O) == ok
        assert lib.fs3_sample_grid(h, C.byref(view(2, 2, 2)), O) == ok

    all_before_the_state_check()
    stale()                                          # 6. before the first step
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


# ---- 7. sampling leaves the state alone ---------------------------------------------------------------------------------------
def test_sampling_leaves_the_state_alone(fs):
    from tests.sample3d_ref import uniform_points
    a, st, off, tick = make_sim(fs, 18 ** 3, fs.FS_MATH_IEEE)
    b, _, _, _ = make_sim(fs, 18 ** 3, fs.FS_MATH_IEEE)
    pts = uniform_points(st, 1000, seed=4)
    for s in range(20):
        a.tick(tick); b.tick(tick)
        if s % 3 == 0:
            assert a.sample(pts)["neighbours"].any()
            a.sample_grid(9, 7, 5)
    assert a.download_particles().tobytes() == b.download_particles().tobytes()
    a.close(); b.close()
