"""CPU-side checks of field sampling (include/fluidsim.h): the checker of tests/sample_checker.cpp is sound on
the oracle's own states (it reproduces every stored density, agrees with a float64 evaluation of the same sums and with a
closed form, and its grid form is its point form on the pixel centres), every host binding names the three calls, fs_sample
is 24 bytes in every layer, and the calls refuse a NULL handle without touching a device.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLE_CALLS = ("fs_sample_points", "fs_sample_points_device", "fs_sample_grid")
EPSILON_F = np.float32(1.19209290e-07)


def make_checker(fs, n, seed, ref_quirks=True):
    from tests.sample_ref import SampleChecker, set_threads
    from tests.track_ref import jitter_velocities
    set_threads(min(8, os.cpu_count() or 1))
    st, off, tick = fs.dam_break_2d(n)
    chk = SampleChecker(st, off, ref_quirks=ref_quirks)
    chk.set_particles(jitter_velocities(chk.particles(), seed))
    return chk, st, tick


def density_identity(samples, particles):
    """fmax(fmax(density, EPSILON), 0.1f), as the density pass clamps, against the stored densities: bitwise."""
    got = np.maximum(np.maximum(samples["density"], EPSILON_F), np.float32(0.1))
    return got.view(np.uint32), particles["density"].view(np.uint32)


@pytest.mark.parametrize("quirks", [0, 1])
@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("n", [4096, 5000])
def test_checker_reproduces_every_stored_density(fs, orc, n, stable, quirks):
    """After 1, 8 and 260 oracle steps: sampling at every predicted position gives every stored density bit for bit through
    the two fmax; with clean cell starts every particle is its own neighbour; the states hold no non-finite value (so nothing is masked anywhere)."""
    chk, _, tick = make_checker(fs, n, seed=n + quirks, ref_quirks=bool(quirks))
    done = 0
    for steps in (1, 8, 260):
        while done < steps:
            chk.step(tick, stable_sort=stable)
            done += 1
        p = chk.particles()
        for f in ("position", "predicted_position", "velocity", "density"):
            assert np.isfinite(p[f]).all(), f"non-finite {f} after {steps} steps"
        out, _ = chk.sample(p["predicted_position"])
        got, want = density_identity(out, p)
        assert np.array_equal(got, want), f"{int((got != want).sum())} of {n} densities differ after {steps} steps"
        assert np.array_equal(out["cell"], p["grid"])
        assert np.isfinite(out["weight"]).all()
        if not quirks:      # (with the stale-start quirk the walk of slot 0's cell may begin past some of its particles)
            assert (out["neighbours"] >= 1).all(), "every particle is its own neighbour"
    chk.close()


def float64_sums(p, start, u, pts, attr=None):
    """O(N * M) evaluation of the statement's sums in float64 over the statement's candidate set: the particles of the valid
    cells of the 3x3 block, from the stored start index on (only the cell of slot 0 can have a stale one), in radius by the
    statement's own f32 test.  -> dict of (sum, sum of absolute terms) per quantity, neighbours, cell."""
    f = np.float32
    gw, gh, n = int(u.grid_w), int(u.grid_h), p.shape[0]
    h, m = f(u.smoothing_radius), float(u.particle_mass)
    h2 = f(h * h)
    cv = float(f(4.0) / (f(np.pi) * f(np.power(np.float32(h), np.float32(8.0)))))
    fx = np.floor((pts[:, 0] + f(u.bounds.x) * f(0.5)) / h)
    fy = np.floor((pts[:, 1] + f(u.bounds.y) * f(0.5)) / h)
    sat = lambda v: np.where(v > 0, np.minimum(v, 4294967295.0), 0).astype(np.uint64)      # noqa: E731
    cx = ((sat(fx.astype(np.float64)) + 1) & 0xFFFFFFFF).astype(np.int64)
    cy = ((sat(fy.astype(np.float64)) + 1) & 0xFFFFFFFF).astype(np.int64)
    pcx, pcy = (p["grid"] % gw).astype(np.int64), (p["grid"] // gw).astype(np.int64)
    slot = np.arange(n)
    cmin = int(p["grid"][0])
    lo_fix = min(int(start[cmin]), int((p["grid"] == cmin).sum()))
    res = []
    for k in range(pts.shape[0]):
        cells = (np.abs(pcx - cx[k]) <= 1) & (np.abs(pcy - cy[k]) <= 1)          # particle cells are valid cells
        dx = p["predicted_position"][:, 0] - pts[k, 0]
        dy = p["predicted_position"][:, 1] - pts[k, 1]
        r2 = dx * dx + dy * dy                                                     # f32, the statement's association
        mask = cells & ~(r2 > h2) & (slot >= lo_fix)
        d = float(h2) - r2[mask].astype(np.float64)
        W = cv * d * d * d
        t = (m / p["density"][mask].astype(np.float64)) * W
        terms = {"density": m * W, "weight": t, "vx": t * p["velocity"][mask, 0], "vy": t * p["velocity"][mask, 1]}
        if attr is not None:
            for c in range(attr.shape[0]):
                terms[f"a{c}"] = t * attr[c, mask]
        res.append(({q: (v.sum(), np.abs(v).sum()) for q, v in terms.items()}, int(mask.sum()),
                    int((cy[k] * gw + cx[k]) & 0xFFFFFFFF)))
    return res


def query_points(st, p, rng):
    """Inside the fluid, in the empty part of the domain, outside the domain."""
    sx, sy = float(st.size.x), float(st.size.y)
    inside = p["predicted_position"][rng.choice(p.shape[0], 150, replace=False)] + rng.uniform(-0.1, 0.1, (150, 2)).astype(np.float32)
    domain = np.stack([rng.uniform(-sx / 2, sx / 2, 150), rng.uniform(-sy / 2, sy / 2, 150)], axis=1)
    outside = np.stack([rng.uniform(-sx, sx, 100), rng.uniform(-sy, sy, 100)], axis=1)
    return np.concatenate([inside, domain, outside]).astype(np.float32)


@pytest.mark.parametrize("quirks", [0, 1])
def test_checker_agrees_with_a_float64_evaluation(fs, orc, quirks):
    """Each f32 sum within 1e-5 of the float64 sum of absolute terms (the project's float contract); neighbours and
    cell exactly.  Channels with mixed signs ride along."""
    n = 5000
    chk, st, tick = make_checker(fs, n, seed=7, ref_quirks=bool(quirks))
    for _ in range(8):
        chk.step(tick)
    rng = np.random.default_rng(3)
    p = chk.particles()
    attr = rng.uniform(-2.0, 2.0, (2, n)).astype(np.float32)
    pts = query_points(st, p, rng)
    out, aout = chk.sample(pts, attr)
    u = fs.Uniform.from_buffer_copy(chk.uniform_bytes())
    ref = float64_sums(p, chk.start_indices(), u, pts, attr)
    hit = 0
    for k, (sums, nb, cell) in enumerate(ref):
        assert int(out["neighbours"][k]) == nb and int(out["cell"][k]) == cell, k
        got = {"density": out["density"][k], "weight": out["weight"][k], "vx": out["velocity"][k, 0], "vy": out["velocity"][k, 1],
               "a0": aout[0, k], "a1": aout[1, k]}
        for q, (s, sabs) in sums.items():
            assert abs(float(got[q]) - s) <= 1e-5 * sabs, (k, q, float(got[q]), s, sabs)
        hit += nb > 0
    assert 150 <= hit < len(ref), "the query set must hit the fluid and miss it"
    chk.close()


def test_two_particles_and_one_point_by_hand(fs, orc):
    """h = 0.5, size 4 x 4 (grid 10 x 10), particles at (0.25, 0.25) and (0.75, 0.25), query at (0.5, 0.25): both at distance
    0.25, r2 = 0.0625, d = 0.1875, W = (1024 / pi) d^3 = 6.75 / pi.  m = 1, densities 2 and 4, velocities (1, 0) and (0, -2):
    density = 2 W, weight = W/2 + W/4, velocity = (W/2, -W/2), one channel {3, -8}: 3 W/2 - 8 W/4 = -W/2.  Cells: the query is
    in (6, 5) = id 56; the particles in ids 55 and 56."""
    from tests.sample_ref import SampleChecker
    f = np.float32
    st = fs.SimulationSettings(2, 0.1, 0.5, (4.0, 4.0), (16, 16))
    chk = SampleChecker(st, ref_quirks=False)
    assert chk.grid_dims == (10, 10)
    chk.begin_tick(fs.default_tick_settings(mass=1.0))
    p = chk.particles_view()
    p["predicted_position"] = [[0.25, 0.25], [0.75, 0.25]]
    p["position"] = p["predicted_position"]
    p["velocity"] = [[1.0, 0.0], [0.0, -2.0]]
    p["density"] = [2.0, 4.0]
    p["grid"] = [55, 56]
    S = chk.start_indices_view()
    S[:] = 0
    S[55], S[56] = 0, 1
    out, aout = chk.sample(np.array([[0.5, 0.25]], dtype=f), np.array([[3.0, -8.0]], dtype=f))
    cv = f(4.0) / (f(np.pi) * f(np.power(f(0.5), f(8.0))))
    W = ((cv * f(0.1875)) * f(0.1875)) * f(0.1875)
    assert out["density"][0] == W + W and out["weight"][0] == f(0.5) * W + f(0.25) * W
    assert out["velocity"][0, 0] == f(0.5) * W and out["velocity"][0, 1] == f(0.0) + f(0.25) * W * f(-2.0)
    assert aout[0, 0] == f(0.5) * W * f(3.0) + f(0.25) * W * f(-8.0)
    assert out["neighbours"][0] == 2 and out["cell"][0] == 56
    assert abs(float(out["density"][0]) - 13.5 / np.pi) < 1e-5 and abs(float(aout[0, 0]) + 3.375 / np.pi) < 1e-5
    # a point two cells away sees nothing; one outside the domain neither, and its cell id is the statement's
    far, _ = chk.sample(np.array([[-1.5, -1.5], [100.0, 0.25]], dtype=f))
    assert not far["neighbours"].any() and not far["density"].any()
    assert far["cell"][1] == 5 * 10 + (int(np.floor((100.0 + 2.0) / 0.5)) + 1)
    chk.close()


def test_checker_grid_is_checker_points_on_the_pixel_centres(fs, orc):
    from tests.sample_ref import grid_points
    chk, st, tick = make_checker(fs, 4096, seed=5)
    for _ in range(4):
        chk.step(tick)
    rng = np.random.default_rng(1)
    attr = rng.uniform(-1.0, 1.0, (3, 4096)).astype(np.float32)
    sx, sy = float(st.size.x), float(st.size.y)
    for (w, h, wmin, wmax) in ((37, 21, (-sx / 2, -sy / 2), (sx / 2, sy / 2)), (16, 50, (-sx, -sy), (sx, sy)),
                               (33, 9, (-1.0, 0.5), (2.5, 3.0))):
        pts = grid_points(w, h, wmin, wmax)
        f = np.float32
        i, j = np.meshgrid(np.arange(w, dtype=f), np.arange(h, dtype=f))
        ex = f(wmin[0]) + ((i + f(0.5)) / f(w)) * (f(wmax[0]) - f(wmin[0]))        # orc_render's expression, f32
        ey = f(wmin[1]) + ((j + f(0.5)) / f(h)) * (f(wmax[1]) - f(wmin[1]))
        assert ex.dtype == f and np.array_equal(pts[:, 0].reshape(h, w), ex) and np.array_equal(pts[:, 1].reshape(h, w), ey)
        g, ga = chk.sample_grid(w, h, wmin, wmax, attr)
        q, qa = chk.sample(pts, attr)
        assert g.tobytes() == q.tobytes() and ga.tobytes() == qa.tobytes()
    assert q["neighbours"].any()
    chk.close()


def test_every_layer_names_every_sampling_call(fs):
    from tests.layers import assert_every_layer_names, header_text
    assert_every_layer_names(fs, SAMPLE_CALLS, fs.FluidSimulation, ("sample", "sample_grid", "sample_device"))
    assert re.search(r"#define\s+FS_ABI_VERSION\s+2\b", header_text())


def test_fs_sample_is_24_bytes_in_every_layer(fs, tmp_path):
    from tests.sample_ref import SAMPLE_DTYPE
    from tests.test_rust_shim import rs_sizeof, rust_structs
    assert C.sizeof(fs._abi.Sample) == 24 and fs.SAMPLE_DTYPE.itemsize == 24
    assert fs.SAMPLE_DTYPE == SAMPLE_DTYPE
    assert [(n, fs.SAMPLE_DTYPE.fields[n][1]) for n in fs.SAMPLE_DTYPE.names] == \
        [("density", 0), ("weight", 4), ("velocity", 8), ("neighbours", 16), ("cell", 20)]
    assert [(n, getattr(fs._abi.Sample, n).offset) for n, _ in fs._abi.Sample._fields_] == \
        [("density", 0), ("weight", 4), ("velocity", 8), ("neighbours", 16), ("cell", 20)]
    rs = rust_structs()
    assert "Sample" in rs, "Rust crate lacks #[repr(C)] Sample"
    assert [f for f, _ in rs["Sample"]] == [f[0] for f in fs._abi.Sample._fields_]
    assert sum(rs_sizeof(t) for _, t in rs["Sample"]) == 24
    src = tmp_path / "probe.c"
    src.write_text('#include "include/fluidsim.h"\n#include <stddef.h>\n'
                   "typedef char a_[sizeof(fs_sample) == 24 ? 1 : -1];\n"
                   "typedef char b_[offsetof(fs_sample, velocity) == 8 && offsetof(fs_sample, neighbours) == 16 && "
                   "offsetof(fs_sample, cell) == 20 ? 1 : -1];\nint main(void) { return 0; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", ROOT, "-c", str(src), "-o", str(tmp_path / "probe.o")])


def test_null_handle_is_invalid_without_a_device(fs):
    lib = fs.load_library()
    inv = fs._abi.FS_ERR_INVALID
    pts = (C.c_float * 8)()
    out = (C.c_uint32 * 24)()
    view = fs._abi.View(fs.Vec2(-1.0, -1.0), fs.Vec2(1.0, 1.0), 2, 2)
    assert lib.fs_sample_points(None, pts, 4, out, None) == inv
    assert b"null" in lib.fs_last_error()
    assert lib.fs_sample_points(None, pts, 0, out, None) == inv
    assert lib.fs_sample_points_device(None, pts, 4, out, None) == inv
    assert lib.fs_sample_grid(None, C.byref(view), out, None) == inv


# ---- the statement itself, restated in plain numpy, against the checker at wrapped and saturated cells --------------------------
from tests import hard_states2d as H  # noqa: E402
from tests import prologue_scenes as S  # noqa: E402

U32 = 0xFFFFFFFF


def _u32_sat(x):
    """NaN and negatives -> 0, >= 2^32 -> 2^32 - 1, else truncation (include/fluidsim.h)"""
    if not (x > 0.0):
        return 0
    if x >= 4294967296.0:
        return U32
    return int(x)


def _powf(x, y):
    """powf of the C library: numpy's float32 power is another implementation and differs from it in the last bit (at h = 0.2,
    0.1, 0.05, 0.33), which would be a difference in Cv and not in the sampler"""
    import ctypes.util
    libm = C.CDLL(ctypes.util.find_library("m"))
    libm.powf.restype, libm.powf.argtypes = C.c_float, [C.c_float, C.c_float]
    return libm.powf(float(x), float(y))


def restated_sample(p, start, u, pts, attr):
    """The statement of include/fluidsim.h "field sampling", line for line: f32 scalars (numpy float32 arithmetic rounds every
    operation to f32 and contracts nothing), one operation per line, the cells of the 3 x 3 block in the statement's order, each
    walked ascending from its stored start index, u32 cell arithmetic wrapping by `& U32`.  Written from the header, not from
    tests/sample_checker.cpp.  -> (SAMPLE_DTYPE[len(pts)], f32 (C, len(pts)))"""
    from tests.sample_ref import SAMPLE_DTYPE
    f = np.float32
    n, gw, gh = int(u.particle_count), int(u.grid_w), int(u.grid_h)
    h, m = f(u.smoothing_radius), f(u.particle_mass)
    h2 = h * h
    h8 = f(_powf(h, 8.0))                                      # powf(h, 8.0f): the C library's, as the header says
    pi_h8 = f(3.14159265) * h8
    cv = f(4.0) / pi_h8
    half_x = f(u.bounds.x) * f(0.5)
    half_y = f(u.bounds.y) * f(0.5)
    grid, q, vel, rho = p["grid"], p["predicted_position"], p["velocity"], p["density"]
    C_ = attr.shape[0]
    out = np.zeros(len(pts), dtype=SAMPLE_DTYPE)
    aout = np.zeros((C_, len(pts)), dtype=f)
    for i, (x, y) in enumerate(pts):
        x, y = f(x), f(y)
        sx = x + half_x
        sy = y + half_y
        qx = sx / h
        qy = sy / h
        cx = (_u32_sat(np.floor(qx)) + 1) & U32
        cy = (_u32_sat(np.floor(qy)) + 1) & U32
        density, weight, vx, vy = f(0.0), f(0.0), f(0.0), f(0.0)
        a = [f(0.0)] * C_
        neighbours = 0
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                X = (cx + ox) & U32
                Y = (cy + oy) & U32
                if X >= gw or Y >= gh:
                    continue
                cid = (Y * gw + X) & U32
                k = int(start[cid])
                while k < n and int(grid[k]) == cid:
                    dx = q[k, 0] - x
                    dy = q[k, 1] - y
                    xx = dx * dx
                    yy = dy * dy
                    r2 = xx + yy
                    if not (r2 > h2):
                        e = h2 - r2
                        w1 = cv * e
                        w2 = w1 * e
                        W = w2 * e
                        mw = m * W
                        density = density + mw
                        mr = m / rho[k]
                        t = mr * W
                        weight = weight + t
                        tx = t * vel[k, 0]
                        ty = t * vel[k, 1]
                        vx = vx + tx
                        vy = vy + ty
                        for c in range(C_):
                            ta = t * attr[c, k]
                            a[c] = a[c] + ta
                        neighbours += 1
                    k += 1
        out[i] = (density, weight, (vx, vy), neighbours, (cy * gw + cx) & U32)
        aout[:, i] = a
    return out, aout


SPECIAL_STATES = {"corners": lambda: S.corners(), "one_cell": lambda: S.one_cell(), "trips2": lambda: S.strip(*S.STRIP["trips2"])}


def _special_state(fs, name):
    """the scene after one oracle step, on the sample checker; two channels with -0.0, denormals and large values"""
    from tests.sample_ref import SampleChecker, set_threads
    set_threads(min(8, os.cpu_count() or 1))
    st, tick, p0 = SPECIAL_STATES[name]()
    chk = SampleChecker(st)
    chk.set_particles(p0)
    chk.step(tick)
    p = chk.particles()
    return chk, st, p, H.sample_channel_values(p.shape[0], 2)


@pytest.mark.parametrize("name", sorted(SPECIAL_STATES))
def test_checker_is_the_statement_at_wrapped_and_saturated_cells(fs, orc, name):
    """The GPU tests of tests/test_sampling_hard_inputs_gpu.py compare the engine with the checker at queries whose cell
    coordinates saturate, wrap to 0 or lie past the grid, at +-inf and NaN.  Here the checker is compared with the plain numpy
    restatement of the header's statement at those queries, on states whose occupied cells include the grid's corners (corners),
    one cell of 256 particles (one_cell) and rows of one particle per cell (trips2): every byte of every sample and channel sum."""
    chk, st, p, attr = _special_state(fs, name)
    pts = H.special_queries(st, p)
    assert 200 <= pts.shape[0] <= 3000
    u = fs.Uniform.from_buffer_copy(chk.uniform_bytes())
    with np.errstate(all="ignore"):
        want, wa = restated_sample(p, chk.start_indices(), u, pts, attr)
    got, ga = chk.sample(pts, attr)
    if got.tobytes() != want.tobytes():
        k = int(np.flatnonzero((got.view(np.uint8).reshape(-1, 24) != want.view(np.uint8).reshape(-1, 24)).any(axis=1))[0])
        raise AssertionError(f"{name}: checker and restatement differ at query {k} {pts[k]}: checker {got[k]}, restatement {want[k]}")
    assert ga.tobytes() == wa.tobytes(), f"{name}: channel sums differ"
    assert got["neighbours"].any() and not got["neighbours"].all()
    chk.close()


def test_special_query_set_reaches_what_it_names(fs, orc):
    """On the checker and the corners scene: a query with neighbours in each of the four corner cells a particle can be in; a
    query whose column wrapped to 0, and one whose row did; a query without a valid column (cx > grid_w), and one without a
    valid row; queries with exactly one valid column (cx == grid_w); NaN, +-inf and -0.0 among the coordinates.  The cell
    coordinates come from tests/pyref.py's xy_of_point, not from the sampler."""
    chk, st, p, attr = _special_state(fs, "corners")
    pts = H.special_queries(st, p)
    out, _ = chk.sample(pts)
    gw, gh = chk.grid_dims
    assert (gw, gh) == S.CORNER_GRID
    cell = H.query_cells(st, pts)
    cx, cy = cell[:, 0], cell[:, 1]
    assert np.array_equal(out["cell"], ((cy * gw + cx) & U32).astype(np.uint32))
    for (x, y) in S.CORNER_CELLS:
        here = (cx == x) & (cy == y)
        assert (out["neighbours"][here] > 0).any(), f"no query with neighbours in corner cell ({x}, {y})"
    big = np.nan_to_num(pts.astype(np.float64), nan=0.0, posinf=1e300, neginf=-1e300)
    assert ((cx == 0) & (big[:, 0] > 1e9) & (cy >= 1) & (cy < gh)).any(), "no query whose column wrapped to 0 in a valid row"
    assert ((cy == 0) & (big[:, 1] > 1e9) & (cx >= 1) & (cx < gw)).any(), "no query whose row wrapped to 0 in a valid column"
    assert ((cx > gw) & (cx < 1000)).any() and ((cy > gh) & (cy < 1000)).any(), "no query just past the last valid column / row"
    assert (cx == gw).any() and (cy == gh).any() and (cx == gw - 1).any() and (cy == gh - 1).any()
    assert not out["neighbours"][(cx > gw) & (cx < 1000)].any()
    assert np.isnan(pts).any() and np.isposinf(pts).any() and np.isneginf(pts).any()
    assert (np.signbit(pts) & (pts == 0)).any()
    assert (np.abs(pts) == np.float32(3e38)).any() and (np.abs(pts) == np.float32(1e10)).any()
    chk.close()
