"""3D surface rendering on the GPU: fs3_render_surface / fs3_render_surface_device against the checker of
tests/render3d_checker.cpp, byte for byte and with no exclusions.  The checker is loaded with the state downloaded from the SAME
handle, so what is compared is the ray-marcher alone, in both math modes; states are asserted finite first.  Particle counts are
the sampler's: 16^3 (whole workgroups) and 18^3 (ragged); images are 64 x 64 (whole workgroups), 37 x 23 (ragged against the
8 x 8 wave tile and the 16 x 16 workgroup), 1 x 1, 65 x 1 and 1 x 65; the march is 64 steps of h / 2."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.bitcmp import assert_identical
from tests.query3d_helpers import checker_of, make_sim
from tests.render3d_ref import Render3Checker

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f = np.float32
SIZES = [(64, 64), (37, 23), (1, 1), (65, 1), (1, 65)]
MAX_STEPS = 64
BOTH = ("ortho_front", "persp_oblique", "persp_fan", "ortho_overhang")        # cameras whose larger images hold hits and misses


def check_views(render, chk, st, p, ctx, sizes=SIZES):
    """Every camera of tests/render3d_ref.py scene_cameras at every size, refine 0 and 8: render(cam, params) against the checker."""
    from tests.render3d_ref import iso_of, params, scene_cameras
    iso = iso_of(p)
    kinds = set()
    for (w, h) in sizes:
        for name, (cam, t_near) in scene_cameras(st, p, w, h).items():
            for refine in (0, 8):
                sp = params(iso, t_near, 0.5 * st.smoothing_radius, MAX_STEPS, refine)
                want = chk.render(cam, sp)
                assert_identical(render(cam, sp), want, f"{ctx}: {name} {w}x{h} refine {refine}")
                kinds.update(np.unique(want["hit"]).tolist())
                if w * h > 65 and name in BOTH:
                    assert (want["hit"] == 1).any() and (want["hit"] == 0).any(), f"{ctx}: {name} {w}x{h}: hits and misses"
                if name == "persp_inside":
                    assert (want["hit"] == 2).all(), f"{ctx}: {name}"
                if name == "persp_away":
                    assert (want["hit"] == 0).all() and (want["steps"] == MAX_STEPS).all(), f"{ctx}: {name}"
    assert kinds == {0, 1, 2}, ctx


def product_render(fs, sim):
    return lambda cam, sp: sim.render_surface(fs.Camera3.from_buffer_copy(bytes(cam)), fs.SurfaceParams3.from_buffer_copy(bytes(sp)))


# ---- 1. shapes and cameras ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ieee", "tolerance"])
@pytest.mark.parametrize("n", [16 ** 3, 18 ** 3])
def test_views_match_checker(fs, n, mode):
    mode = fs.FS_MATH_IEEE if mode == "ieee" else fs.FS_MATH_TOLERANCE
    sim, st, off, tick = make_sim(fs, n, mode)
    done = 0
    for steps in (1, 8, 60):
        while done < steps:
            sim.tick(tick)
            done += 1
        chk, p = checker_of(Render3Checker, sim, st, off, tick.mass)
        check_views(product_render(fs, sim), chk, st, p, f"n {n} mode {mode} step {steps}")
        chk.close()
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
    chk, p = checker_of(Render3Checker, sim, st, off, heavy.mass)
    check_views(product_render(fs, sim), chk, st, p, f"mass 1.5 mode {mode}", sizes=SIZES[1:])
    chk.close()
    sim.tick(tick)                                  # the mass of the LAST step is what counts
    chk, p = checker_of(Render3Checker, sim, st, off, tick.mass)
    check_views(product_render(fs, sim), chk, st, p, f"mass back to 1 mode {mode}", sizes=SIZES[1:])
    chk.close(); sim.close()


# ---- 3. dense cluster: long row ranges ----------------------------------------------------------------------------------------
def test_dense_cluster(fs):
    from tests.render3d_ref import camera, params
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
    chk, q = checker_of(Render3Checker, sim, st, off, tick.mass)
    assert sim.sample(q["predicted_position"])["neighbours"].max() > 700
    render = product_render(fs, sim)
    c = lo.astype(np.float64) + [h, 0.5 * h, 0.5 * h]
    # a quarter of the cluster's central density: the few lattice particles left around it stay far below it
    iso = 0.25 * float(sim.sample(c[None, :].astype(np.float32))["density"][0])
    for refine in (0, 8):
        for w, hh in ((37, 23), (16, 16)):
            cam = camera(c - [0, 0, 6 * h], [0, 0, 1], [5 * h * w / hh, 0, 0], [0, 5 * h, 0], w, hh, True)
            sp = params(iso, 0.0, 0.5 * h, MAX_STEPS, refine)
            want = chk.render(cam, sp)
            assert (want["hit"] == 1).any() and (want["hit"] == 0).any()
            assert_identical(render(cam, sp), want, f"cluster ortho {w}x{hh} refine {refine}")
            cam = camera(c - [2 * h, 1 * h, 5 * h], [0.4, 0.2, 1], [1.2 * w / hh, 0, 0], [0, 1.2, 0], w, hh, False)
            want = chk.render(cam, sp)
            assert (want["hit"] == 1).any() and (want["hit"] == 0).any()
            assert_identical(render(cam, sp), want, f"cluster perspective {w}x{hh} refine {refine}")
    chk.close(); sim.close()


# ---- 4. tie to the public sampler (no checker) --------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ieee", "tolerance"])
def test_hits_are_the_public_samplers_records(fs, mode):
    from tests.render3d_ref import iso_of, params, points_at, scene_cameras
    mode = fs.FS_MATH_IEEE if mode == "ieee" else fs.FS_MATH_TOLERANCE
    sim, st, off, tick = make_sim(fs, 18 ** 3, mode)
    for _ in range(8):
        sim.tick(tick)
    p = sim.download_particles()
    render = product_render(fs, sim)
    seen = 0
    for name, (cam, t_near) in scene_cameras(st, p, 37, 23).items():
        for refine in (0, 8):
            got = render(cam, params(iso_of(p), t_near, 0.5 * st.smoothing_radius, MAX_STEPS, refine))
            hit = got["hit"] != 0
            if not hit.any():
                continue
            seen += int(hit.sum())
            S = sim.sample(points_at(cam, got["t"])[hit])
            assert np.array_equal(S["density"].view(np.uint32), got["density"][hit].view(np.uint32)), name
            assert (S["density"] >= f(iso_of(p))).all(), name
            with np.errstate(all="ignore"):
                g = S["gradient"]
                gl = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]).astype(f)
                normal = np.where(gl[:, None] > 0, (-g) / gl[:, None], f(0)).astype(f)
                vel = np.where(S["weight"][:, None] > 0, S["velocity"] / S["weight"][:, None], f(0)).astype(f)
            assert np.array_equal(normal.view(np.uint32), got["normal"][hit].view(np.uint32)), name
            assert np.array_equal(vel.view(np.uint32), got["velocity"][hit].view(np.uint32)), name
    assert seen > 500
    sim.close()


# ---- 5. device form, stream-ordered between steps -----------------------------------------------------------------------------
DEVICE_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r)
import torch                                   # torch FIRST: one HIP runtime per process
import numpy as np
import gpu_fluid_simulation_amd as g
from tests.render3d_ref import iso_of, params, scene_cameras
from tests.track_ref import jitter_velocities
n, w, h = 18 ** 3, 37, 23
st, off, tick = g.dam_break_3d(n)
dev = torch.device("cuda", 0)
def make():
    sim = g.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.upload_particles(jitter_velocities(sim.download_particles(), 7))
    return sim
ref = make()
ref.tick(tick)
p0 = ref.download_particles()
views = []
for name in ("ortho_front", "persp_oblique"):
    cam, t_near = scene_cameras(st, p0, w, h)[name]
    views.append((g.Camera3.from_buffer_copy(bytes(cam)), g.SurfaceParams3(iso_of(p0), t_near, 0.5 * st.smoothing_radius, 64, 8)))
sim = make()
assert sim.stream_ptr
ext = torch.cuda.ExternalStream(sim.stream_ptr, device=dev)
outs = []
with torch.cuda.stream(ext):
    for k in range(4):
        outs.append(torch.zeros(w * h * 10, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    # step, render, step, render: no host synchronisation in between
    for k in range(2):
        for _ in range(1 if k == 0 else 4):
            sim.tick(tick)
        for v, (cam, sp) in enumerate(views):
            assert sim.render_surface(cam, sp, out=outs[2 * k + v].data_ptr()) is None
sim.sync()
got = [o.cpu().numpy().tobytes() for o in outs]
for k in range(2):                             # re-run to each rendered step for the blocking form
    if k == 1:
        for _ in range(4):
            ref.tick(tick)
    for v, (cam, sp) in enumerate(views):
        want = ref.render_surface(cam, sp)
        assert (want["hit"] == 1).any() and (want["hit"] == 0).any()
        assert got[2 * k + v] == want.tobytes(), "device render %%d of step %%d differs from the blocking form" %% (v, 1 + 4 * k)
assert got[0] != got[2], "the two rendered states must differ"
assert sim.download_particles().tobytes() == ref.download_particles().tobytes()
print("DEVICE_OK")
"""


def test_device_form_between_steps(fs):
    out = subprocess.run([sys.executable, "-c", DEVICE_SCRIPT % {"root": ROOT}], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "DEVICE_OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


# ---- 6. checks, in the order of the header --------------------------------------------------------------------------------------
def test_checks_in_the_headers_order_and_state_guards(fs):
    lib = fs.load_library()
    inv, ok = fs._abi.FS_ERR_INVALID, fs._abi.FS_OK
    sim, st, off, tick = make_sim(fs, 16 ** 3, fs.FS_MATH_IEEE)          # created and uploaded to: no step yet
    h = sim._h
    good_cam = fs.look_at_camera((0, 0, -3), (0, 0, 0), (0, -1, 0), 0.8, 5, 4)
    good = fs.SurfaceParams3(1.0, 0.0, 0.1, 16, 4)
    out = np.zeros((4, 5), dtype=fs.SURFACE_HIT_DTYPE)
    O = out.ctypes.data
    err = lambda: lib.fs_last_error().decode()                                                   # noqa: E731
    calls = (lib.fs3_render_surface, lib.fs3_render_surface_device)      # the device form is refused before `out` is touched

    def cam_with(**kw):
        c = fs.Camera3.from_buffer_copy(good_cam)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def sp_with(**kw):
        s = fs.SurfaceParams3.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    bad_cams = [cam_with(width=0), cam_with(height=0), cam_with(width=1 << 13, height=(1 << 13) + 1), cam_with(width=0xFFFFFFFF, height=0xFFFFFFFF),
                cam_with(reserved=1), cam_with(orthographic=2), cam_with(orthographic=-1)]
    nan, inf = float("nan"), float("inf")
    bad_sps = [sp_with(iso=0.0), sp_with(iso=-1.0), sp_with(iso=nan), sp_with(iso=inf), sp_with(t_near=-0.5), sp_with(t_near=nan),
               sp_with(t_near=inf), sp_with(ds=0.0), sp_with(ds=-0.1), sp_with(ds=nan), sp_with(ds=inf), sp_with(max_steps=0),
               sp_with(max_steps=4097), sp_with(refine=25)]

    def refused(call, cam, sp, o, text):
        status = call(h, C.byref(cam) if cam is not None else None,
                      C.byref(sp) if sp is not None else None, o)
        assert status == inv and text in err(), (status, err(), text)

    def all_before_the_state_check():
        for call in calls:
            # 1. NULL handle (before anything else), camera, params, out
            assert call(None, C.byref(bad_cams[0]), C.byref(bad_sps[0]), None) == inv and "null" in err()
            refused(call, None, good, O, "null")
            refused(call, good_cam, None, O, "null")
            refused(call, good_cam, good, None, "null")
            refused(call, bad_cams[0], bad_sps[0], None, "null")
            # 2. the camera, before the params
            for c in bad_cams:
                refused(call, c, bad_sps[0], O, "image size" if c.reserved == 0 and c.orthographic in (0, 1) else "camera")
            # 3. the params
            for s in bad_sps:
                refused(call, good_cam, s, O, "surface params")
            refused(call, good_cam, sp_with(max_steps=4096, refine=24, iso=-1.0), O, "iso")

    def stale():
        for call in calls:
            refused(call, good_cam, good, O, "needs a step")
            refused(call, good_cam, bad_sps[0], O, "surface params")         # 3 before 4

    def valid():
        assert lib.fs3_render_surface(h, C.byref(good_cam), C.byref(good), O) == ok
        assert lib.fs3_render_surface(h, C.byref(cam_with(orthographic=1)), C.byref(sp_with(max_steps=4096, refine=24, t_near=0.0)), O) == ok
        assert lib.fs3_render_surface(h, C.byref(cam_with(width=1, height=1)), C.byref(sp_with(max_steps=1, refine=0)), O) == ok

    all_before_the_state_check()
    stale()                                          # 4. before the first step
    assert not out.view(np.uint8).any()
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


# ---- 7. rendering leaves the state alone --------------------------------------------------------------------------------------
def test_rendering_leaves_the_state_alone(fs):
    a, st, off, tick = make_sim(fs, 18 ** 3, fs.FS_MATH_IEEE)
    b, _, _, _ = make_sim(fs, 18 ** 3, fs.FS_MATH_IEEE)
    from tests.render3d_ref import iso_of
    iso = None
    for s in range(20):
        a.tick(tick); b.tick(tick)
        if s % 3 == 0:
            iso = iso or iso_of(a.download_particles())
            cam = fs.look_at_camera((-2.5, -1.5, -3.0), (-0.8, 0.2, 0.0), (0, -1, 0), 0.9, 37, 23, orthographic=bool(s % 2))
            assert (a.render_surface(cam, fs.SurfaceParams3(iso, 0.0, 0.1, 64, 4))["hit"] != 0).any()
    assert a.download_particles().tobytes() == b.download_particles().tobytes()
    a.close(); b.close()
