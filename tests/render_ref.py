"""Independent float64 restatement of the density-splat fragment shader (fluid_shader.wgsl:27-102), written from the
shader text as a specification.  TEST INFRASTRUCTURE ONLY.  It pins both the kernel (k_render_density) and the C++
oracle (orc_render), and shares no code with either.

What it takes from f32 and what it does not:
  * The pixel's point and its home cell are f32, operation by operation: the point by the mapping include/fluidsim.h
    states for fs_view, the cell by funcs.wgsl:212-214 (floor((p + bounds * 0.5) / h), saturating f32 -> u32, + 1).
    The 5x5 window is a hard cut and the cut depends on the cell, so a float64 cell would be a different image.
  * Everything after the home cell is float64: distances, exp, length, log, the smoothsteps, the mix.  The shader's
    literals (0.01, 0.7, ...) are f32 in WGSL and enter as the f32 values they round to.

Candidates are found by brute force: every particle whose STORED cell id (x = id % grid_w, y = id / grid_w) lies in the
window (u32(cx + ox), u32(cy + oy)), ox, oy in -2..2, and in the grid (x < grid_w, y < grid_h: a window cell beyond
that is the wrapped / out-of-range id that holds nothing, include/fluidsim.h).  The start indices are not walked, so
the cell table and the kernel's merged row ranges are not trusted; the records must be in the order a step leaves
them (ascending cell id), which render_ref asserts.

The one thing the start indices decide: compute.wgsl:45-56 never writes the start of the cell of sorted
index 0, cell c0 = particles[0].grid, so the shader walks that cell from the stale value v = start_indices[c0] and sees
its particles [min(v, cnt), cnt) only (cnt = number of particles in c0, which occupy [0, cnt)).  The particles of sorted
index < min(v, cnt) are hidden from every pixel: hidden_by_stale_start() names them and render_ref leaves them out."""
import numpy as np

f32 = np.float32
# struct Uniforms, funcs.wgsl:17-51 (120 bytes)
UNIFORM_DTYPE = np.dtype([("delta", "<f4"), ("particle_count", "<u4"), ("sqr_radius", "<f4"), ("frame_time", "<u4"),
                          ("gravity", "<f4", (2,)), ("bounds", "<f4", (2,)), ("mouse_pos", "<f4", (2,)),
                          ("smoothing_radius", "<f4"), ("particle_mass", "<f4"), ("pressure_constant", "<f4"),
                          ("rest_density", "<f4"), ("damping_factor", "<f4"), ("viscosity_coefficient", "<f4"),
                          ("surface_tension_treshold", "<f4"), ("surface_tension_coefficient", "<f4"),
                          ("poly6_kernel_volume", "<f4"), ("poly6_kernel_derivative", "<f4"), ("poly6_kernel_laplacian", "<f4"),
                          ("spiky_kernel_derivative", "<f4"), ("viscosity_kernel", "<f4"), ("mouse_state", "<i4"),
                          ("mouse_force_radius", "<f4"), ("mouse_force_power", "<f4"), ("grid_w", "<u4"), ("grid_h", "<u4"),
                          ("texture_size", "<f4", (2,))])
assert UNIFORM_DTYPE.itemsize == 120

EPS23 = 2.0 ** -23
M32 = 0xFFFFFFFF


def parse_uniform(uniform):
    """The 120 bytes of the uniform (bytes, or the ctypes struct of the product ABI) -> one UNIFORM_DTYPE record."""
    raw = uniform if isinstance(uniform, (bytes, bytearray)) else bytes(uniform)
    assert len(raw) == 120
    return np.frombuffer(raw, dtype=UNIFORM_DTYPE)[0]


def pixel_points(width, height, world_min, world_max):
    """f32 (height, width) x and y of the pixel centres: world_min + ((i + 0.5) / width, (j + 0.5) / height) * (world_max - world_min)."""
    wmin = (f32(world_min[0]), f32(world_min[1]))
    wmax = (f32(world_max[0]), f32(world_max[1]))
    fx = (np.arange(width, dtype=f32) + f32(0.5)) / f32(width)
    fy = (np.arange(height, dtype=f32) + f32(0.5)) / f32(height)
    x = wmin[0] + fx * (wmax[0] - wmin[0])
    y = wmin[1] + fy * (wmax[1] - wmin[1])
    assert x.dtype == f32 and y.dtype == f32
    return np.broadcast_to(x[None, :], (height, width)), np.broadcast_to(y[:, None], (height, width))


def _u32_sat(v):
    """WGSL u32(f32): saturating, NaN -> 0.  int64 out."""
    v = np.asarray(v, dtype=np.float64)
    out = np.zeros(v.shape, dtype=np.int64)
    pos = v > 0.0
    big = v >= 4294967296.0
    out[pos & ~big] = v[pos & ~big].astype(np.int64)
    out[big] = M32
    return out


def home_cells(u, px, py):
    """funcs.wgsl:212-214 in f32: (cx, cy) as int64 holding the wrapped u32 values."""
    h = f32(u["smoothing_radius"])
    bx, by = f32(u["bounds"][0]), f32(u["bounds"][1])
    with np.errstate(over="ignore", invalid="ignore"):
        qx = np.floor((px + bx * f32(0.5)) / h)
        qy = np.floor((py + by * f32(0.5)) / h)
    assert qx.dtype == f32 and qy.dtype == f32
    return (_u32_sat(qx) + 1) & M32, (_u32_sat(qy) + 1) & M32


def hidden_by_stale_start(particles, start_indices, uniform):
    """Sorted indices of the particles the stale start of the first sorted cell hides from the shader (module docstring)."""
    u = parse_uniform(uniform)
    grid = particles["grid"].astype(np.int64)
    n = int(u["particle_count"])
    if n == 0 or grid[0] >= start_indices.shape[0]:
        return np.zeros(0, dtype=np.int64)
    c0 = int(grid[0])
    cnt = int(np.count_nonzero(grid[:n] == c0))
    assert (grid[:cnt] == c0).all(), "the records are not in cell order"
    return np.arange(min(int(start_indices[c0]), cnt), dtype=np.int64)


def _smoothstep(a, b, x):
    a, b = np.float64(f32(a)), np.float64(f32(b))
    t = np.clip((x - a) / (b - a), 0.0, 1.0)
    return t * t * (3.0 - 2.0 * t)


def shade(density, vsum):
    """fluid_shader.wgsl:78-101 in float64: (density, sum of contrib * |v|) -> RGBA (..., 4)."""
    vf = vsum * np.float64(f32(0.01))
    vf = np.log(1.0 + 5.0 * vf) / np.log(1.0 + 5.0)
    vf = np.clip(vf, 0.0, 1.0)
    interior = _smoothstep(0.5, 1.5, density)
    edge = _smoothstep(0.7, 1.0, density) - _smoothstep(1.0, 1.5, density)
    edge = edge * (1.0 + vf * 2.0)
    out = np.empty(density.shape + (4,), dtype=np.float64)
    blue, red = (0.0, 0.5, 1.0), (1.0, 0.0, 0.0)
    for c in range(3):
        out[..., c] = (blue[c] * (1.0 - vf) + red[c] * vf) * interior + edge
    out[..., 3] = np.clip(interior, 0.0, 1.0)
    return out


def render_ref(particles, start_indices, uniform, width, height, world_min, world_max, stale_start=True, chunk=1024):
    """-> (rgba float64 (height, width, 4), density float64 (height, width), candidates int64 (height, width)).
    particles: PARTICLE_DTYPE records in the order a step leaves them; start_indices: the u32 table; uniform: 120 bytes or
    the ctypes struct.  stale_start=False shows what the image would be if the stale start hid nothing."""
    u = parse_uniform(uniform)
    n = int(u["particle_count"])
    gw, gh = int(u["grid_w"]), int(u["grid_h"])
    p = particles[:n]
    grid = p["grid"].astype(np.int64)
    assert (np.diff(grid) >= 0).all(), "the records are not in cell order: no step since the last upload?"
    seen = grid < gw * gh                               # an id beyond the table is never a window cell of the grid
    if stale_start:
        seen[hidden_by_stale_start(p, start_indices, uniform)] = False
    gx, gy = (grid % gw)[seen], (grid // gw)[seen]
    q = p["predicted_position"][seen].astype(np.float64)
    speed = np.hypot(*p["velocity"][seen].astype(np.float64).T)
    px, py = pixel_points(width, height, world_min, world_max)
    cx, cy = home_cells(u, px, py)
    px, py, cx, cy = (a.reshape(-1) for a in (px, py, cx, cy))
    npix = width * height
    density, vsum, cand = np.zeros(npix), np.zeros(npix), np.zeros(npix, dtype=np.int64)
    denom = np.float64(f32(u["sqr_radius"])) / 2.0      # fluid_shader.wgsl:66
    for a in range(0, npix, chunk):
        s = slice(a, min(a + chunk, npix))
        # x == u32(cx + ox) for an ox in -2..2  <=>  (x - cx + 2) mod 2^32 <= 4; the particle's x < grid_w is the grid test
        win = (((gx[None, :] - cx[s, None] + 2) & M32) <= 4) & (((gy[None, :] - cy[s, None] + 2) & M32) <= 4)
        pi, qi = np.nonzero(win)
        dx = q[qi, 0] - np.float64(px[s][pi])
        dy = q[qi, 1] - np.float64(py[s][pi])
        contrib = np.exp(-(dx * dx + dy * dy) / denom)
        m = s.stop - s.start
        density[s] = np.bincount(pi, weights=contrib, minlength=m)
        vsum[s] = np.bincount(pi, weights=contrib * speed[qi], minlength=m)
        cand[s] = np.bincount(pi, minlength=m)
    density, vsum, cand = (a.reshape(height, width) for a in (density, vsum, cand))
    return shade(density, vsum), density, cand


def f32_sum_bound(density, cand):
    """Per pixel, what an in-order f32 evaluation of the shader may differ from render_ref by, on any channel:
         15 * (N + 8) * 2^-23 * max(1, density)  +  4 * 2^-23 * 3
    N f32 additions of non-negative terms lose at most N * 2^-24 of the running sum each way, the terms themselves (a
    subtraction, two squares, an add, a division, exp: ~8 roundings, exp's own 1-2 ulp included) another 8 * 2^-24 relative;
    2^-23 instead of 2^-24 leaves the speed-weighted sum its share.  That is the density's error; smoothstep(0.7, 1.0, .) has
    slope 5 and the edge term is scaled by up to 3, so a colour moves by up to 15 x as much.  The second term is the last
    colour arithmetic: ~4 roundings on values up to 3."""
    return 15.0 * (cand + 8.0) * EPS23 * np.maximum(1.0, density) + 4.0 * EPS23 * 3.0
