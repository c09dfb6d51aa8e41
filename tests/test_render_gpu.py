"""Renderer hand-off: the headless density-splat image (k_render_density) against the oracle's restatement of
fluid_shader.wgsl:27-102 (orc_render) AND against the independent float64 restatement tests/render_ref.py on the handle's own
downloaded state.  exp / log are device-library functions, so the bar is a float tolerance, derived and not guessed:
  * kernel vs oracle: render_scenes.oracle_bound(scene) = max(4 * D_scene, 16 * 2^-23), D_scene being the ORACLE's measured
    f32-vs-f64 deviation (tests/test_render.py) — nothing the GPU computed enters it;
  * kernel vs float64: render_ref.f32_sum_bound per pixel, 15 (N + 8) 2^-23 max(1, density) + 12 * 2^-23.
In FS_MATH_IEEE the handle's state is the oracle's bit for bit (asserted); in the other math modes it is not, and the oracle
is given the handle's downloaded records and start indices before it renders."""
import ctypes as C

import numpy as np
import pytest

from tests import render_ref as R
from tests import render_scenes as S

pytestmark = pytest.mark.gpu


def make_pair(fs, orc, scene, counting=False, math="FS_MATH_IEEE", quirks=True, steps=None, **kw):
    sim = fs.FluidSimulation(scene.settings, device=0, initial_offset=scene.offset, ref_quirks=quirks, math_mode=getattr(fs, math),
                             sort_mode=fs.FS_SORT_COUNTING if counting else fs.FS_SORT_BITONIC, **kw)
    ref = orc.OracleSim(scene.settings, scene.offset, ref_quirks=quirks)
    if scene.prepare is not None:
        p = scene.prepare(ref.particles())
        ref.set_particles(p); sim.upload_particles(p)
    for _ in range(scene.steps if steps is None else steps):
        sim.tick(scene.tick); ref.step(scene.tick, stable_sort=counting)
    return sim, ref


def same_state(sim, ref, exact):
    """-> the handle's (records, start indices, uniform); afterwards the oracle holds that very state."""
    p, si, u = sim.download_particles(), sim.download_start_indices(), sim.uniform()
    for f in ("position", "predicted_position", "velocity", "density"):
        assert np.isfinite(p[f]).all()
    if exact:
        assert p.tobytes() == ref.particles().tobytes() and np.array_equal(si, ref.start_indices()), "parity lost: not a renderer matter"
    else:
        ref.set_particles(p)
        ref.start_indices_view()[:] = si
    return p, si, u


def check_views(sim, ref, scene_name, views, ctx, exact=True):
    p, si, u = same_state(sim, ref, exact)
    tol = S.oracle_bound(scene_name)
    out = {}
    for name, (w, h, wmin, wmax) in views.items():
        got = sim.render_density(w, h, wmin, wmax)
        assert got.shape == (h, w, 4) and got.dtype == np.float32
        want = ref.render(w, h, wmin, wmax)
        want64, density, cand = R.render_ref(p, si, u, w, h, wmin, wmax)
        eo = np.abs(got.astype(np.float64) - want).max(axis=-1)
        e64 = np.abs(got - want64).max(axis=-1)
        bound = R.f32_sum_bound(density, cand)
        ko, k64 = np.unravel_index(np.argmax(eo), eo.shape), np.unravel_index(np.argmax(e64 - bound), e64.shape)
        print(f"{ctx}/{name}: vs oracle {eo.max():.3e} (bound {tol:.3e}); vs float64 {e64.max():.3e}, worst err/bound {np.max(e64 / bound):.3f}")
        assert eo.max() <= tol, f"{ctx}/{name}: pixel {ko}: kernel {got[ko]}, oracle {want[ko]}, bound {tol:.3e}"
        assert (e64 <= bound).all(), f"{ctx}/{name}: pixel {k64}: kernel {got[k64]}, float64 {want64[k64]}, bound {bound[k64]:.3e}, N {cand[k64]}"
        out[name] = got
    return out


def test_density_splat_matches_oracle(fs, orc, tmp_path):
    st, off, tick = fs.dam_break_2d(4096)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    ref = orc.OracleSim(st, off)
    with pytest.raises(fs.FluidSimError):
        sim.render_density(8, 8)                         # no cell table before the first step
    for _ in range(40):
        sim.tick(tick); ref.step(tick)
    wmin, wmax = (-st.size.x / 2, -st.size.y / 2), (st.size.x / 2, st.size.y / 2)
    got = sim.render_density(160, 100)
    want = ref.render(160, 100, wmin, wmax)
    assert got.shape == (100, 160, 4)
    np.testing.assert_allclose(got, want, rtol=0, atol=S.oracle_bound("dam"))
    assert got[..., 3].max() == 1.0 and got[..., 3].min() == 0.0      # fluid and empty space both visible
    # zoomed view + PNG writer
    z = sim.render_density(64, 64, world_min=(-6.4, 2.0), world_max=(-4.4, 4.0))
    np.testing.assert_allclose(z, ref.render(64, 64, (-6.4, 2.0), (-4.4, 4.0)), rtol=0, atol=S.oracle_bound("dam"))
    path = tmp_path / "frame.png"
    fs.write_png(str(path), got)
    assert path.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"


# ---- 1. sort modes, math modes, quirks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("quirks", [True, False])
@pytest.mark.parametrize("math", ["FS_MATH_IEEE", "FS_MATH_WGSL_ULP", "FS_MATH_TOLERANCE"])
@pytest.mark.parametrize("counting", [False, True])
def test_modes(fs, orc, counting, math, quirks):
    sc = S.dam()
    sim, ref = make_pair(fs, orc, sc, counting=counting, math=math, quirks=quirks)
    views = {k: sc.views[k] for k in ("domain", "zoom")}
    img = check_views(sim, ref, "dam", views, f"dam counting={counting} {math} quirks={quirks}", exact=math == "FS_MATH_IEEE")
    a = img["domain"][..., 3]
    assert a.max() == 1.0 and a.min() == 0.0 and ((a > 0) & (a < 1)).mean() > 0.05
    sim.close()


@pytest.mark.parametrize("counting", [False, True])
def test_mass_other_than_one_on_a_non_square_domain(fs, orc, counting):
    """particle_mass = 1.5: the density lives in rho2 / the keys in the pairs in another way than with the default mass."""
    sc = S.random()
    assert sc.tick.mass == 1.5 and sc.settings.size.x != sc.settings.size.y
    sim, ref = make_pair(fs, orc, sc, counting=counting)
    img = check_views(sim, ref, "random", sc.views, f"random counting={counting}")
    assert img["domain"][..., :3].max() > 1.5
    sim.close()


# ---- 2. the stale start of the first sorted cell ----------------------------------------------------------------------------
def test_poisoned_stale_start(fs, orc):
    """The step setup of test_parity_gpu.py::test_poisoned_stale_start.  The kernel's merged row range with `a == 0 -> lo_fix`
    must hide exactly the particles the shader's per-cell walk does not see."""
    sc = S.stale()
    sim, ref = make_pair(fs, orc, sc)
    for v in S.STALE_POISON:
        c0 = S.poison(ref, v, sim)
        sim.tick(sc.tick); ref.step(sc.tick)
        p, si, u = ref.particles(), ref.start_indices(), ref.uniform_bytes()
        # the precondition, from the references alone
        assert int(p["grid"][0]) == c0 and int(si[c0]) == v
        assert R.hidden_by_stale_start(p, si, u).size >= 1
        views = S.stale_views(sc.settings, c0, ref.grid_dims[0])
        w, h, wmin, wmax = views["zoom"]
        with_, density, cand = R.render_ref(p, si, u, w, h, wmin, wmax)
        without, _, _ = R.render_ref(p, si, u, w, h, wmin, wmax, stale_start=False)
        moved = np.abs(with_ - without).max(axis=-1)
        assert (moved > 100 * R.f32_sum_bound(density, cand)).any() and moved.max() > 100 * S.oracle_bound("stale")
        check_views(sim, ref, "stale", views if v == S.STALE_POISON[0] else {"zoom": views["zoom"]}, f"stale v={v}")
    sim.close()


# ---- 3. views that leave the domain -------------------------------------------------------------------------------------------
def test_views_that_leave_the_domain(fs, orc):
    sc = S.outside()
    sim, ref = make_pair(fs, orc, sc)
    gw, gh = ref.grid_dims
    grid = ref.particles()["grid"]
    assert (grid % gw == gw - 1).any() and (grid // gw == gh - 1).any(), "the last column and row must hold particles"
    img = check_views(sim, ref, "outside", sc.views, "outside")
    assert not img["beyond"].any()                                   # colour 0, alpha 0
    for name in ("left", "right", "above", "below", "overhang", "far"):
        a = img[name][..., 3]
        assert a.max() == 1.0 and a.min() == 0.0, name
    assert (img["point"] == img["point"][0, 0]).all() and img["point"][0, 0, 3] > 0
    sim.close()


# ---- 4. launch shapes -----------------------------------------------------------------------------------------------------------
def test_launch_shapes(fs, orc):
    sc = S.dam()
    sim, ref = make_pair(fs, orc, sc)
    views = {k: sc.views[k] for k in ("129x65", "1x300", "257x1", "1x1")}
    assert all((w * h) % 256 != 0 for (w, h, _, _) in views.values())
    img = check_views(sim, ref, "dam", views, "shapes")
    assert img["1x300"][..., 3].max() == 1.0 and img["257x1"][..., 3].max() == 1.0 and img["1x1"][0, 0, 3] > 0
    sim.close()


# ---- 5. features on; the renderer changes nothing ---------------------------------------------------------------------------
def test_surface_tension_and_tracking_do_not_change_the_image(fs, orc):
    """Tracking (2 channels) on, and surface tension enabled with a threshold no normal reaches (a zero force: the step is the
    plain one, test_surface_tension_gpu.py): the image is the plain handle's, byte for byte.  With the default threshold the
    state is another one, and the image is the references' of THAT state."""
    sc = S.random()
    sc.tick.surface_tension_treshold = float("inf")
    plain, ref = make_pair(fs, orc, sc)
    want = plain.render_density(*sc.views["domain"])
    assert want[..., 3].max() == 1.0
    trk, _ = make_pair(fs, orc, sc, track=2)
    assert trk.render_density(*sc.views["domain"]).tobytes() == want.tobytes()
    both, _ = make_pair(fs, orc, sc, track=2, surface_tension=True)
    assert both.surface_tension_enabled and both.track_channels == 2
    a, b = both.download_particles(), plain.download_particles()
    assert all(np.array_equal(a[f], b[f]) for f in a.dtype.names)
    assert both.render_density(*sc.views["domain"]).tobytes() == want.tobytes()
    sc = S.random()
    st_on, ref2 = make_pair(fs, orc, sc, track=2, surface_tension=True)
    assert st_on.surface_tension_forces().any()
    check_views(st_on, ref2, "random", {"129x65": sc.views["129x65"]}, "surface tension on", exact=False)
    for s in (plain, trk, both, st_on):
        s.close()


@pytest.mark.parametrize("counting", [False, True])
def test_rendering_leaves_the_state_alone(fs, orc, counting):
    sc = S.random()
    a, _ = make_pair(fs, orc, sc, counting=counting, steps=0, track=1)
    b, _ = make_pair(fs, orc, sc, counting=counting, steps=0, track=1)
    for s in range(12):
        a.tick(sc.tick); b.tick(sc.tick)
        if s % 3 == 0:
            a.render_density(33, 19)
        if s % 5 == 0:
            a.render_density(129, 65, (-6.0, -5.0), (6.0, 5.0))
    before = (a.download_particles().tobytes(), a.download_start_indices().tobytes())
    one = a.render_density(129, 65)
    two = a.render_density(129, 65)
    assert one.tobytes() == two.tobytes() and one[..., 3].any()
    assert (a.download_particles().tobytes(), a.download_start_indices().tobytes()) == before
    assert before == (b.download_particles().tobytes(), b.download_start_indices().tobytes())
    assert a.particle_ids().tobytes() == b.particle_ids().tobytes()
    a.close(); b.close()


# ---- 6. the state guard --------------------------------------------------------------------------------------------------------
def test_render_is_refused_between_an_upload_and_the_next_step(fs, orc):
    """fs_upload_particles writes the records in upload order under the previous sort's cell table: a render would walk old
    ranges over re-ordered arrays.  It is refused (as sampling is) until the next step, and right after that step."""
    sc = S.dam(steps=5)
    sim, ref = make_pair(fs, orc, sc)
    inv = fs._abi.FS_ERR_INVALID
    view = sc.views["129x65"]
    sim.render_density(*view)
    rng = np.random.default_rng(3)
    p = ref.particles()
    shuffled = p[rng.permutation(p.shape[0])]
    for what in ("full", "partial", "start_indices"):
        if what == "full":
            sim.upload_particles(shuffled); ref.set_particles(shuffled)
        elif what == "partial":
            q = ref.particles()
            q[:1000] = q[:1000][::-1]
            sim.upload_particles(q[:1000]); ref.set_particles(q)
        else:
            si = ref.start_indices()
            si[int(ref.particles()["grid"][0])] = 1
            sim.upload_start_indices(si); ref.start_indices_view()[:] = si
        for _ in range(2):                                # ... and keeps being refused
            with pytest.raises(fs.FluidSimError) as e:
                sim.render_density(*view)
            assert e.value.status == inv, what
        sim.tick(sc.tick); ref.step(sc.tick)
        check_views(sim, ref, "dam", {"129x65": view}, f"after {what} upload")
    sim.close()


def test_render_is_refused_on_a_dead_handle_and_on_a_slab_handle(fs, monkeypatch):
    """After a reported sort barrier time-out (the setup of test_sort_gpu.py::test_a_barrier_time_out_report_kills_the_handle,
    which needs its particle count: the stand-by kernel) the order is undefined: render reports FS_ERR_DEVICE."""
    n = 1 << 18
    monkeypatch.setenv("FS_SORT_TRUST", "1")
    monkeypatch.setenv("FS_SORT_INJECT_TIMEOUT", "1")
    st, off, tick = fs.dam_break_2d(n)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    monkeypatch.delenv("FS_SORT_TRUST")
    monkeypatch.delenv("FS_SORT_INJECT_TIMEOUT")
    rng = np.random.default_rng(11)
    sim.upload_particles(sim.download_particles()[rng.permutation(n)])
    sim.tick(tick)                                        # the stand-by kernel runs (and "times out") in this very step
    for _ in range(2):
        with pytest.raises(fs.FluidSimError) as e:
            sim.render_density(33, 19)
        assert e.value.status == fs._abi.FS_ERR_DEVICE and "timed out" in str(e.value)
    assert sim.sort_plan()["timeouts"] >= 1
    del sim
    st2, _, _ = fs.dam_break_2d(16384)
    slab = fs.SlabSimulation(st2, 10, 40, False, False, 16384 + 2 * 2048, 2048, 66, device=0)
    view = fs._abi.View(fs.Vec2(-1.0, -1.0), fs.Vec2(1.0, 1.0), 2, 2)
    out = np.zeros(16, dtype=np.float32)
    assert fs.load_library().fs_render_density(slab._h, C.byref(view), out.ctypes.data_as(C.c_void_p)) == fs._abi.FS_ERR_UNSUPPORTED
    slab.close()
