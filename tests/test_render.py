"""Pins the oracle's density-splat image (orc_render in oracle/sph_oracle.cpp) against the independent float64 restatement of
fluid_shader.wgsl:27-102 in tests/render_ref.py, and measures D_scene, the oracle's f32-vs-f64 deviation that the GPU tests'
kernel-vs-oracle bound is derived from (tests/render_scenes.py D_SCENE).  No GPU.

The bound asserted per pixel is render_ref.f32_sum_bound (derived there): 15 (N + 8) 2^-23 max(1, density) + 12 * 2^-23."""
import numpy as np
import pytest

from tests import render_ref as R
from tests import render_scenes as S


def compare(ref, views, ctx):
    """-> D: max abs deviation of the oracle's image from the float64 one, over the views; asserts the derived bound per pixel."""
    p, si, u = ref.particles(), ref.start_indices(), ref.uniform_bytes()
    for f in ("predicted_position", "velocity"):
        assert np.isfinite(p[f]).all()
    D = 0.0
    for name, (w, h, wmin, wmax) in views.items():
        want, density, cand = R.render_ref(p, si, u, w, h, wmin, wmax)
        got = ref.render(w, h, wmin, wmax).astype(np.float64)
        err = np.abs(got - want).max(axis=-1)
        bound = R.f32_sum_bound(density, cand)
        k = np.unravel_index(np.argmax(err - bound), err.shape)
        print(f"{ctx}/{name}: max abs {err.max():.3e}, worst err/bound {np.max(err / bound):.3f}, candidates <= {cand.max()}")
        assert (err <= bound).all(), f"{ctx}/{name}: pixel {k}: oracle {got[k]}, float64 {want[k]}, bound {bound[k]:.3e}, N {cand[k]}"
        D = max(D, float(err.max()))
    return D


def check_recorded(scene, D):
    print(f"D_scene[{scene}] = {D:.3e} (recorded {S.D_SCENE[scene]:.1e})")
    assert S.D_SCENE[scene] / 2 < D <= S.D_SCENE[scene], "tests/render_scenes.py D_SCENE and DESIGN.md §15 hold another value"


def test_dam_break(orc):
    sc = S.dam()
    ref = S.build_oracle(orc, sc)
    img = ref.render(*sc.views["domain"])
    assert img[..., 3].max() == 1.0 and img[..., 3].min() == 0.0 and ((img[..., 3] > 0) & (img[..., 3] < 1)).mean() > 0.05
    check_recorded("dam", compare(ref, sc.views, "dam"))


def test_random_state_on_a_non_square_domain(orc):
    sc = S.random()
    ref = S.build_oracle(orc, sc)
    assert ref.grid_dims == (47, 37)
    img = ref.render(*sc.views["domain"])
    assert ((img[..., 3] > 0) & (img[..., 3] < 1)).mean() > 0.03 and img[..., :3].max() > 1.5      # the ramp and the edge highlight
    check_recorded("random", compare(ref, sc.views, "random"))


def test_poisoned_stale_start(orc):
    """A non-zero stale start under the first sorted cell: the particles it hides are missing from the oracle's image, and the
    image would be another one if they were not."""
    sc = S.stale()
    ref = S.build_oracle(orc, sc)
    D = 0.0
    for v in S.STALE_POISON:
        c0 = S.poison(ref, v)
        ref.step(sc.tick)
        p, si, u = ref.particles(), ref.start_indices(), ref.uniform_bytes()
        assert int(p["grid"][0]) == c0 and int(si[c0]) == v, "the first sorted cell moved: the poison is not under it"
        hidden = R.hidden_by_stale_start(p, si, u)
        assert hidden.size >= 1
        views = S.stale_views(sc.settings, c0, ref.grid_dims[0])
        w, h, wmin, wmax = views["zoom"]
        with_, density, cand = R.render_ref(p, si, u, w, h, wmin, wmax)
        without, _, _ = R.render_ref(p, si, u, w, h, wmin, wmax, stale_start=False)
        moved = np.abs(with_ - without).max(axis=-1)
        assert (moved > 100 * R.f32_sum_bound(density, cand)).any(), "hiding the particles changes no pixel: the case proves nothing"
        D = max(D, compare(ref, views, f"stale v={v}"))
    check_recorded("stale", D)


def test_views_that_leave_the_domain(orc):
    sc = S.outside()
    ref = S.build_oracle(orc, sc)
    gw, gh = ref.grid_dims
    grid = ref.particles()["grid"]
    assert (grid % gw == gw - 1).any() and (grid // gw == gh - 1).any() and (grid % gw == 1).any() and (grid // gw == 1).any()
    assert not ref.render(*sc.views["beyond"]).any()
    for name in ("left", "right", "above", "below", "overhang"):
        a = ref.render(*sc.views[name])[..., 3]
        assert a.max() == 1.0 and a.min() == 0.0, name
    pt = ref.render(*sc.views["point"])
    assert (pt == pt[0, 0]).all() and pt[0, 0, 3] > 0
    fl, ov = ref.render(*sc.views["flipped"]), ref.render(*sc.views["overhang"])
    assert np.abs(fl[::-1, ::-1] - ov).max() < 1e-3 and not np.array_equal(fl[::-1, ::-1], ov)
    check_recorded("outside", compare(ref, sc.views, "outside"))


def test_reference_window_is_a_hard_cut(orc):
    """What the float64 restatement is for: a candidate two cells away is taken, three cells away is not, whatever its distance."""
    sc = S.dam(steps=1)
    ref = S.build_oracle(orc, sc)
    p, si, u = ref.particles(), ref.start_indices(), ref.uniform_bytes()
    uu = R.parse_uniform(u)
    gw, h = int(uu["grid_w"]), float(uu["smoothing_radius"])
    q = p["predicted_position"][2000].astype(np.float64)
    gx = int(p["grid"][2000]) % gw
    x_in = (gx + 2 - 1 + 0.5) * h - float(uu["bounds"][0]) / 2       # a point whose cell is gx + 2 ... gx + 3
    for cells, expect in ((2, True), (3, False)):
        x = x_in + (cells - 2) * h
        _, density, cand = R.render_ref(p, si, u, 1, 1, (x, q[1]), (x, q[1]))
        alone = p.copy()
        alone["predicted_position"][2000] = (1e3, 1e3)              # the same records with that particle far away, cell id unchanged
        _, d2, c2 = R.render_ref(alone, si, u, 1, 1, (x, q[1]), (x, q[1]))
        assert (cand[0, 0] - c2[0, 0] == 0) and (density[0, 0] > d2[0, 0]) == expect
