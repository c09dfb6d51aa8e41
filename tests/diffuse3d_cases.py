"""What tests/test_diffusion3d.py (CPU) and tests/test_diffusion3d_gpu.py share: the scenes by name, the channel contents, how a
conductivity is chosen from the checker alone, the plan a scene runs with, and the comparison of a handle with its checker.
TEST INFRASTRUCTURE ONLY; no pytest mark."""
import numpy as np

import paths3d
from oracle import oracle as O
from tests import bitcmp
from tests import diffuse3d_ref as DR
from tests import track3d_ref as TR

f32 = np.float32
NONVACUOUS = ["dam16", "pair12"] + sorted(paths3d.scenes())


def scene_state(fs, name):
    """(settings, tick, records, steps) of a scene by name: "dam16" (the 16^3 dam break with jittered velocities), "pair12"
    (paths3d.pair3_state(side 12)) or a scene of paths3d.scenes()"""
    if name == "dam16":
        st, off, tick = fs.dam_break_3d(4096)
        ref = O.OracleSim3D(st, off)
        p = TR.jitter_velocities3(ref.particles(), 12)
        ref.close()
        return st, tick, p, 3
    if name == "pair12":
        ref, st, tick, p = paths3d.pair3_state(fs, O, 12)
        ref.close()
        return st, tick, p, 3
    scene = paths3d.scenes()[name]
    st, tick, p = paths3d.build_state(fs, scene)
    return st, tick, p, max(scene.steps, 3)


def fill_channels(rec, channels, seed=0):
    """(channels, n) f32: position x, position y scaled to 1e3, finite values up to 1e30 of both signs, position z"""
    n = rec.shape[0]
    rng = np.random.default_rng(100 + seed)
    rows = [rec["position"][:, 0], rec["position"][:, 1] * f32(1e3),
            (rng.uniform(-1.0, 1.0, n) * 10.0 ** rng.uniform(-3, 30, n)).astype(f32), rec["position"][:, 2]]
    return np.ascontiguousarray(np.stack(rows[:channels]).astype(f32))


def clone(chk):
    """a checker of its own with the records, ids, channels, settings and tick count of `chk`"""
    out = DR.Diffuse3Checker(chk.settings, channels=chk.channels, tick_count=chk.tick_count)
    out.set_particles(chk.particles())
    out.ids, out.attr = chk.ids.copy(), chk.attr.copy()
    out.kappa, out.buoyancy, out.surface_tension = list(chk.kappa), chk.buoyancy, chk.surface_tension
    return out


def pass_of_next_step(chk, tick):
    """the pass of the step to come, on a scratch copy: R and the channels it will read"""
    probe = clone(chk)
    probe.step(tick)
    out = dict(R=probe.R.copy(), attr=probe.attr_in.copy())
    probe.close()
    return out


def kappa_for(R, delta, target):
    """the conductivity at which g R = target at the slot where R is largest, g = (2 kappa) delta; rounded down to f32"""
    k = f32(target / (2.0 * float(delta) * float(np.max(R))))
    while (f32(2.0) * k) * f32(delta) * np.max(R) > target:
        k = np.nextafter(k, f32(0.0))
    return float(k)


SUBSETS = [(0,), (1, 3), (0, 1, 2), (0, 1, 2, 3)]
SCENE_STEPS = 3


def scene_plan(name):
    """(diffusing subset, buoyancy) a path scene runs with: the subset and the buoyancy channel — inside or outside it, never the
    channel of values to 1e30, whose force would throw the feature out of its cells — go round by scene"""
    k = sorted(paths3d.scenes()).index(name)
    return SUBSETS[k % 4], ((0, 1, 3)[k % 3], 0.25, 0.1)


def restatement(chk, rec, attr, mass, g):
    """The pass in float64 over every ordered pair within h (the pairs come from a k-d tree, a superset filtered by the
    statement's own f32 test) on the records after a checker step — their predicted positions and densities are what the pass
    read.  q, r2 and d are the statement's f32 values; everything behind them is float64.
    -> (A' [N], sum_j |term_ij| [N], K [N], R [N])"""
    from scipy.spatial import cKDTree
    h = f32(chk.settings.smoothing_radius)
    h2 = f32(h * h)
    cg = float(f32(6.0) * f32(chk.constants()[0]))
    q32 = np.ascontiguousarray(rec["predicted_position"], dtype=f32)
    n = q32.shape[0]
    nb = cKDTree(q32.astype(np.float64)).query_ball_point(q32.astype(np.float64), float(h) * (1 + 1e-5))
    i = np.repeat(np.arange(n), [len(x) for x in nb])
    j = np.concatenate([np.asarray(x, dtype=np.int64) for x in nb])
    o = q32[j] - q32[i]
    r2 = o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1] + o[:, 2] * o[:, 2]
    near = ~(r2 > h2)
    i, j, r2 = i[near], j[near], r2[near]
    d = (h2 - r2).astype(np.float64)
    rho = rec["density"].astype(np.float64)
    wk = (float(f32(mass)) / rho[j]) * (cg * d * d)
    a = attr.astype(np.float64)
    t = wk * (a[j] - a[i])
    acc, tabs = np.bincount(i, t, n), np.bincount(i, np.abs(t), n)
    K = np.bincount(i, minlength=n)
    u = 1.0 / rho
    return a + float(g) * acc * u, float(g) * tabs * u, K, u * np.bincount(i, wk, n)


class Planned:
    pass


def planned_run(fs, name, channels=1):
    """one step of a scene on the checker alone with channel 0 = position x diffusing at g R = 1/2 and as the buoyancy channel
    about its median: the shares the non-vacuity test asserts"""
    st, tick, p, _ = scene_state(fs, name)
    chk = DR.Diffuse3Checker(st, channels=channels)
    chk.set_particles(p)
    chk.attr[:] = fill_channels(p, channels)
    probe = pass_of_next_step(chk, tick)
    run = Planned()
    run.n = chk.n
    run.kappa = kappa_for(probe["R"], tick.delta, 0.5)
    chk.kappa[0] = run.kappa
    a0 = float(np.median(chk.attr[0]))
    chk.buoyancy = (0, 0.25, a0)
    chk.step(tick)
    moved = bitcmp.bits(chk.attr[0]) != bitcmp.bits(chk.attr_in[0])
    # a slot has a neighbour when some candidate but itself is inside the radius: its weight sum exceeds its own term's
    rho = chk.particles_view()["density"].astype(np.float64)
    own = (float(tick.mass) / rho) * (1.0 / rho) * float(f32(6.0) * f32(chk.constants()[0])) * \
        float(f32(st.smoothing_radius) * f32(st.smoothing_radius)) ** 2
    paired = chk.R > own * (1 + 1e-6)
    s = 0.25 * (a0 - chk.attr_in[0].astype(np.float64))
    run.moved_all = float(moved.mean())
    run.paired = int(paired.sum())
    run.moved_paired = float(moved[paired].mean()) if run.paired else 0.0
    run.s_pos, run.s_neg = int((s > 0).sum()), int((s < 0).sum())
    assert np.isfinite(chk.fb).all() and (chk.fb != 0).any()
    chk.close()
    return run


# ---- a handle against its checker -------------------------------------------------------------------------------------------------
def same_vec3(got, want, ctx):
    ok = bitcmp.same_words(got, want)
    assert ok.all(), f"{ctx}: {int((~ok).sum())} words differ; first slot {int(np.argmax(~ok.all(axis=1)))}"


def assert_same(sim, chk, ctx):
    """ids, every channel, fb, every float of the state and the keys: bit for bit, a NaN met by any NaN"""
    bitcmp.assert_records_equal(sim.download_particles(), chk.particles(), ctx, nan_any=True)
    bitcmp.assert_track_equal(sim, chk, ctx, nan_any=True)
    if chk.buoyancy is not None:
        same_vec3(sim.buoyancy_forces(), chk.fb, ctx + ": fb")
    if chk.surface_tension is not None:
        same_vec3(sim.surface_tension_forces(), chk.st, ctx + ": st")


def configure(sim, chk, kappa=None, buoyancy="keep", surface_tension="keep"):
    """the same settings into the handle and its checker.  kappa: {channel: conductivity}; buoyancy: (channel, beta, A0) or None;
    surface_tension: (sigma, tau) or None"""
    for c, k in (kappa or {}).items():
        sim.set_diffusion(c, k)
        chk.kappa[c] = float(f32(k))
    if buoyancy != "keep":
        if buoyancy is None:
            sim.clear_buoyancy()
        else:
            sim.set_buoyancy(*buoyancy)
        chk.buoyancy = buoyancy
    if surface_tension != "keep":
        if surface_tension is None:
            sim.clear_surface_tension()
        else:
            sim.set_surface_tension(*surface_tension)
        chk.surface_tension = surface_tension


def set_channels(sim, chk, values):
    values = np.ascontiguousarray(values, dtype=np.float32)
    for c in range(chk.channels):
        sim.set_attribute(c, values[c])
    chk.attr = values.copy()


def make_pair(fs, st, p, channels, math_mode=None, capacity=None):
    """(handle, checker) holding the records p, tracking on with `channels` channels"""
    kw = {} if math_mode is None else dict(math_mode=math_mode)
    sim = fs.FluidSimulation3D(st, device=0, **kw)
    if capacity:
        sim.reserve(capacity)
    sim.upload_particles(p)
    sim.track(channels)
    chk = DR.Diffuse3Checker(st, channels=channels)
    chk.set_particles(p)
    return sim, chk
