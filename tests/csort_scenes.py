"""Scenes that put FS_SORT_COUNTING (csrc/kernels_csort.hip, csrc/fs_scan.h) on its edges — TEST INFRASTRUCTURE, plain numpy.

Crafted positions choose the cell keys, so a scene decides how many particles share a cell (CS_RANK_MAX = 2048 separates the serial
rank loop from the in-place segment sort), where the cell's slots [lo, hi) sit among k_cs_fixreorder's 256-slot workgroups, how
long the cell table is (k_scan_lookback: 16 items per thread, 16384 per tile, 64 tiles per look-back trip) and which key runs the
lanes of a wave see in the histogram (wave_run / cell_ticket).

Every builder returns (settings, tick, particles, facts).  `facts` is what the scene is MEANT to hit, computed here on the CPU
from the f32 predicted positions with tests/pyref.py's xy_of_point; tests/test_csort_scenes.py asserts it without a GPU, and
tests/test_csort_gpu.py runs the same scenes on the engine.  Builders are cached: treat what they return as read-only.

Placement rules: h = 0.2, a roomy box; a particle sits at a distinct random point 0.01 .. 0.19 inside its cell and moves less
than 0.001 in the predict step, so it keeps its cell; the members of a cell come from scattered source indices, so the order in
which the histogram atomics are served cannot be the source order by construction."""
import functools

import numpy as np

import gpu_fluid_simulation_amd as g
from tests import pyref

f32 = np.float32
H = 0.2
RANK_MAX = 2048                  # CS_RANK_MAX
GROUP = 256                      # CS_BLOCK: slots per k_cs_fixreorder workgroup
SCAN_ITEMS, SCAN_TILE = 16, 16384
BOX = (40.0, 30.0)               # 202 x 152 cells
VEL = 0.05


def default_tick():
    return g.default_tick_settings(gravity=(0.0, 9.81))


def predicted(particles, settings, tick):
    """compute.wgsl:8-30 in f32."""
    dt = f32(tick.delta)
    pred = (particles["position"] + particles["velocity"] * dt).astype(f32)
    bs = np.array([f32(settings.size.x) * f32(0.5), f32(settings.size.y) * f32(0.5)], dtype=f32)
    return np.where(np.abs(pred) > bs, bs * np.sign(pred), pred).astype(f32)


def cpu_keys(particles, settings, tick):
    gw, gh = formula_grid(settings)
    u = {"bounds": (f32(settings.size.x), f32(settings.size.y)), "h": f32(settings.smoothing_radius)}
    out = np.empty(particles.shape[0], dtype=np.uint32)
    for i, pt in enumerate(predicted(particles, settings, tick)):
        cx, cy = pyref.xy_of_point(u, pt)
        out[i] = (cy * gw + cx) & 0xFFFFFFFF
    return out


def formula_grid(settings):
    """grid_dims: ceil(size / h) + 2 per axis, the division in f32."""
    h = f32(settings.smoothing_radius)
    return (int(np.ceil(f32(settings.size.x) / h)) + 2, int(np.ceil(f32(settings.size.y) / h)) + 2)


def stable_perm(keys):
    return np.argsort(keys, kind="stable").astype(np.uint32)


def make_facts(settings, tick, particles, **extra):
    keys = cpu_keys(particles, settings, tick)
    gw, gh = formula_grid(settings)
    n = keys.shape[0]
    cells, counts = np.unique(keys, return_counts=True)
    lo = np.concatenate([[0], np.cumsum(counts)[:-1]])
    big = [{"key": int(k), "m": int(c), "lo": int(a), "hi": int(a + c), "lo_mod": int(a % GROUP)}
           for k, c, a in zip(cells, counts, lo) if c > RANK_MAX]
    perm = stable_perm(keys)
    count = gw * gh + 1
    facts = {"n": n, "keys": keys, "grid": (gw, gh), "cells": cells, "counts": counts, "big": big,
             "scan_count": count, "scan_tiles": -(-count // SCAN_TILE), "perm": perm,
             "moved": float((perm != np.arange(n)).mean())}
    facts.update(extra)
    return facts


def cell_origin(settings, cx, cy):
    return np.array([(cx - 1) * H - settings.size.x / 2, (cy - 1) * H - settings.size.y / 2])


def fill(particles, idx, settings, cells, rng):
    """Put particle idx[j] at a random point inside cells[j] = (cx, cy)."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 2)
    org = (cells - 1) * H - np.array([settings.size.x / 2, settings.size.y / 2])
    particles["position"][idx] = (org + rng.uniform(0.01, 0.19, size=(len(idx), 2))).astype(f32)


def sparse_cells(rng, count, cx_range, cy_range, per_cell=3):
    """`count` cell coordinates drawn from the rectangle, at most `per_cell` (<= 4) in any one cell."""
    xs, ys = np.arange(*cx_range), np.arange(*cy_range)
    k = -(-count // per_cell)
    assert k <= xs.size * ys.size, "rectangle too small"
    pick = rng.choice(xs.size * ys.size, k, replace=False)
    cells = np.stack([xs[pick % xs.size], ys[pick // xs.size]], axis=1)
    return cells[np.arange(count) % k]


def finish(settings, particles, rng, vel=VEL):
    n = particles.shape[0]
    particles["predicted_position"] = particles["position"]
    particles["velocity"] = rng.uniform(-vel, vel, size=(n, 2)).astype(f32)
    particles["density"] = 0
    particles["grid"] = 0
    assert np.unique(particles["position"], axis=0).shape[0] == n, "coincident points"
    return particles


# ---- one / two / all: big cells among the 256-slot workgroups -----------------------------------------------------------
BIG_ROW = 76                     # the big cell's row in the 202 x 152 grid; rows below hold lower keys, rows above higher ones


@functools.lru_cache(maxsize=None)
def one_cell(m, before, after, seed=1):
    """One cell of m particles; `before` particles in lower-keyed cells (<= 4 per cell, so lo == before), `after` in higher ones."""
    n = before + m + after
    st, tick = g.SimulationSettings(n, 0.1, H, BOX), default_tick()
    rng = np.random.default_rng(seed + 7919 * m + before)
    p = np.zeros(n, dtype=g.PARTICLE_DTYPE)
    src = rng.permutation(n)                                      # = rng.choice without replacement, for every group
    fill(p, src[:m], st, [(100, BIG_ROW)] * m, rng)
    fill(p, src[m:m + before], st, sparse_cells(rng, before, (1, 201), (1, BIG_ROW)), rng)
    fill(p, src[m + before:], st, sparse_cells(rng, after, (1, 201), (BIG_ROW + 1, 151)), rng)
    p = finish(st, p, rng)
    return st, tick, p, make_facts(st, tick, p, m=m, before=before, after=after)


@functools.lru_cache(maxsize=None)
def two_cells(m_a, m_b, before, n=8192, seed=2):
    """Two cells with consecutive occupied keys (hi_a == lo_b) that are no geometric neighbours: 4 rows apart, the rows between
    them and the rest of their own rows empty, so the force pass visits m_a^2 + m_b^2 pairs, not (m_a + m_b)^2."""
    after = n - before - m_a - m_b
    assert after >= 0
    st, tick = g.SimulationSettings(n, 0.1, H, BOX), default_tick()
    rng = np.random.default_rng(seed + 7919 * m_a + 104729 * m_b + before)
    p = np.zeros(n, dtype=g.PARTICLE_DTYPE)
    src = rng.permutation(n)
    fill(p, src[:m_a], st, [(150, BIG_ROW)] * m_a, rng)
    fill(p, src[m_a:m_a + m_b], st, [(50, BIG_ROW + 4)] * m_b, rng)
    o = m_a + m_b
    fill(p, src[o:o + before], st, sparse_cells(rng, before, (1, 201), (1, BIG_ROW)), rng)
    fill(p, src[o + before:], st, sparse_cells(rng, after, (1, 201), (BIG_ROW + 5, 151)), rng)
    p = finish(st, p, rng)
    return st, tick, p, make_facts(st, tick, p, m_a=m_a, m_b=m_b, before=before, after=after)


@functools.lru_cache(maxsize=None)
def all_in_one(n, seed=3):
    st, tick = g.SimulationSettings(n, 0.1, H, BOX), default_tick()
    rng = np.random.default_rng(seed + n)
    p = np.zeros(n, dtype=g.PARTICLE_DTYPE)
    fill(p, np.arange(n), st, [(100, BIG_ROW)] * n, rng)
    p = finish(st, p, rng)
    return st, tick, p, make_facts(st, tick, p, m=n)


# ---- small and ragged n: the jittered lattice of test_counting_sort_mode_matches_stable_oracle, source order shuffled ----
@functools.lru_cache(maxsize=None)
def lattice(n):
    side = float(np.ceil(np.sqrt(n))) * 0.1
    st, tick = g.SimulationSettings(n, 0.1, H, (2.0 * side, 1.5 * side)), default_tick()
    rng = np.random.default_rng(1000 + n)
    lat = g.reference_lattice(st, (0.0, 0.0))
    lat["position"] += rng.uniform(-0.025, 0.025, size=(n, 2)).astype(f32)
    lat["predicted_position"] = lat["position"]
    lat["velocity"] = rng.uniform(-1, 1, size=(n, 2)).astype(f32)
    # the lattice's own order is nearly cell order for a handful of particles: draw source orders until the stable permutation
    # moves more than half the slots (any order does at the larger n)
    for _ in range(64):
        p = lat[rng.permutation(n)]
        keys = cpu_keys(p, st, tick)
        if np.unique(keys).size == 1 or (stable_perm(keys) != np.arange(n)).mean() > 0.5:
            break
    return st, tick, p, make_facts(st, tick, p)


# ---- the scan's table ----------------------------------------------------------------------------------------------------
def exact_side(cells):
    """A box side s (f32) with s / h == cells exactly in f32: grid_dims gives cells + 2, and a particle clamped to +s/2 lands in
    the last reachable cell, cells + 1."""
    h = f32(H)
    for toward in (f32(0), f32(np.inf)):
        s = f32(cells) * h
        for _ in range(8):
            if f32(s / h) == f32(cells):
                return float(s)
            s = np.nextafter(s, toward)
    raise AssertionError(f"no f32 side gives {cells} cells")


@functools.lru_cache(maxsize=None)
def table(gw, gh, n=3000, seed=4):
    """gw x gh cells and n sparse particles: one in the lowest reachable cell (cx = cy = 1), one in the highest (gw - 1, gh - 1,
    clamped to +bounds / 2: the last key of the table), cells occupied in the first and the last scan tile, and — where the
    table has more than 65 tiles — a stretch of at least 64 tiles in between without a particle."""
    size = (exact_side(gw - 2), exact_side(gh - 2))
    st, tick = g.SimulationSettings(n, 0.1, H, size), default_tick()
    assert formula_grid(st) == (gw, gh)
    rng = np.random.default_rng(seed + 31 * gw + gh)
    p = np.zeros(n, dtype=g.PARTICLE_DTYPE)
    tiles = -(-(gw * gh + 1) // SCAN_TILE)
    body = n - 2
    if tiles > 65:             # a band of rows inside the first tile; the last tile (a row or less) holds the corner particle
        rows = SCAN_TILE // gw - 1
        cells = sparse_cells(rng, body, (1, gw - 1), (1, 1 + rows))
        if tiles > 130:        # and half of them in a band that starts in tile 66: tiles 1 .. 65 stay empty
            r0 = 66 * SCAN_TILE // gw + 1
            cells[::2] = sparse_cells(rng, len(cells[::2]), (1, gw - 1), (r0, r0 + 8))
    else:
        cells = sparse_cells(rng, body, (1, gw - 1), (1, gh - 1))
    src = rng.permutation(n)
    fill(p, src[:body], st, cells, rng)
    p["position"][src[body]] = (-size[0] / 2, -size[1] / 2)
    p["position"][src[body + 1]] = (size[0] / 2, size[1] / 2)
    p = finish(st, p, rng)
    p["velocity"][src[body]] = (-VEL, -VEL)                       # both leave the box in the predict step and are clamped
    p["velocity"][src[body + 1]] = (VEL, VEL)
    facts = make_facts(st, tick, p, corner_lo=int(src[body]), corner_hi=int(src[body + 1]))
    occ = np.zeros(facts["scan_tiles"], dtype=bool)
    occ[facts["cells"] // SCAN_TILE] = True
    gaps = np.diff(np.concatenate([[-1], np.nonzero(occ)[0], [occ.size]])) - 1
    facts["tile_occupied"], facts["longest_empty_tiles"] = occ, int(gaps.max())
    return st, tick, p, facts


# ---- key runs across the lanes of a wave ----------------------------------------------------------------------------------
def _runs_labels(pattern):
    A, B, C, D, E = range(5)
    if pattern == "full_wave":                # one run fills a wave; the same key again two waves on
        return [A] * 64 + [B] * 64 + [A] * 64 + [C] * 64
    if pattern == "ends_at_63":               # a run ends at lane 63 and a NEW key starts at lane 0 of the next wave
        return [A] * 40 + [B] * 24 + [C] * 10 + [D] * 54 + [E] * 64
    if pattern == "continues":                # the same key goes on across the wave boundary, twice, once over a whole wave
        return [A] * 30 + [B] * 34 + [B] * 20 + [C] * 44 + [C] * 64 + [C] * 5 + [D] * 59
    if pattern == "alternating":              # every lane its own run: 64 atomics per wave, two keys
        return [A, B] * 64 + [C, D] * 32 + [A] * 64
    if pattern == "lengths_1_to_64":          # run lengths 1, 2, ..., 64 one after the other, 40 keys taking turns
        return [k % 40 for k in range(1, 65) for _ in range(k)]
    if pattern == "ragged_1":                 # n % 64 == 1: the last wave has one active lane, its key continues from lane 63
        return [A] * 64 + [A] * 30 + [B] * 34 + [B]
    if pattern == "ragged_63":                # n % 64 == 63: a run ends at the last active lane, lane 62
        return [A] * 64 + [B] * 64 + [C] * 20 + [D] * 43
    raise KeyError(pattern)


RUN_PATTERNS = ("full_wave", "ends_at_63", "continues", "alternating", "lengths_1_to_64", "ragged_1", "ragged_63")


def lane_runs(keys):
    """[(wave, first lane, length, key)] as wave_run sees them: runs of equal keys inside each 64-lane wave."""
    out = []
    for w in range(0, len(keys), 64):
        k = keys[w:w + 64]
        cut = np.concatenate([[0], np.nonzero(k[1:] != k[:-1])[0] + 1, [len(k)]])
        out += [(w // 64, int(a), int(b - a), int(k[a])) for a, b in zip(cut[:-1], cut[1:])]
    return out


@functools.lru_cache(maxsize=None)
def runs(pattern, seed=5):
    """Source order = the pattern's label sequence; label j sits in a cell of its own, later labels in LOWER keys, so the sort
    turns the order of the runs around."""
    labels = np.array(_runs_labels(pattern))
    n = labels.size
    st, tick = g.SimulationSettings(n, 0.1, H, BOX), default_tick()
    rng = np.random.default_rng(seed + n)
    nl = int(labels.max()) + 1
    assert nl <= 40
    cell_of = np.stack([190 - 4 * np.arange(nl), np.full(nl, 100)], axis=1)
    p = np.zeros(n, dtype=g.PARTICLE_DTYPE)
    fill(p, np.arange(n), st, cell_of[labels], rng)
    p = finish(st, p, rng)
    facts = make_facts(st, tick, p, labels=labels)
    facts["lane_runs"] = lane_runs(facts["keys"])
    return st, tick, p, facts


# ---- a slab scene: two big cells, one interior and one at the rank boundary ------------------------------------------------
def still_tick():
    """Force terms that vanish exactly: the pressure and viscosity constants are 0, so a step is v += g dt, x += v dt."""
    return g.default_tick_settings(gravity=(0.0, 9.81), pressure_constant=0.0, viscosity_coefficient=0.0)


@functools.lru_cache(maxsize=None)
def slab_two_big_cells(n=16384, m=2500, col_a=30, col_b=90, world=2, seed=6):
    """World 2.  Background: the same number of particles in every column 1 .. 200, one per cell; cell A (m particles) in column
    col_a, deep inside rank 0; cell B in column col_b, which the equal-count partition makes the LAST column of rank 0: B is
    owned by rank 0, sent to rank 1 as halo and therefore sorted on both ranks, among the edge columns / boundary strips."""
    from gpu_fluid_simulation_amd import multi
    st, tick = g.SimulationSettings(n, 0.1, H, BOX), still_tick()
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=g.PARTICLE_DTYPE)
    src = rng.permutation(n)
    fill(p, src[:m], st, [(col_a, 40)] * m, rng)
    fill(p, src[m:2 * m], st, [(col_b, 110)] * m, rng)
    body = n - 2 * m
    cols = 1 + np.arange(body) % 200
    rows = np.empty(body, dtype=np.int64)
    for c in range(1, 201):
        sel = cols == c
        free = np.setdiff1d(np.arange(1, 151), [40] if c == col_a else [110] if c == col_b else [])
        rows[sel] = rng.choice(free, int(sel.sum()), replace=False)
    fill(p, src[2 * m:], st, np.stack([cols, rows], axis=1), rng)
    p = finish(st, p, rng)
    facts = make_facts(st, tick, p, m=m)
    gw = facts["grid"][0]
    colx = multi.global_columns(p["position"][:, 0], st.size.x, st.smoothing_radius)
    hist = np.bincount(colx, minlength=gw)[:gw]
    facts["bounds"] = multi.partition_columns(hist, world)
    facts["col_a"], facts["col_b"] = col_a, col_b
    return st, tick, p, facts


# ---- the cases both test files run: tests/test_csort_scenes.py proves the edge, tests/test_csort_gpu.py runs the engine ------
N_BIG = 8192
# rank bound (2047 / 2048 rank loop, 2049 sorted) and the network's sizes: p2 == m at 4096, p2 = 8192 at 4097, p2 = 16384 at 8193
RANK_CASES = [(m, 1000, N_BIG - 1000 - m) for m in (2047, 2048, 2049, 4095, 4096, 4097)] + [(8193, 1000, 12288 - 1000 - 8193)]
# (m, before, after, lo % 256, hi == n): the segment's first slot first / second / last in its workgroup; the segment ends the
# array, with n a multiple of 256 and one more
PLACEMENT_CASES = [(2049, 1024, N_BIG - 1024 - 2049, 0, False), (2049, 1025, N_BIG - 1025 - 2049, 1, False),
                   (2049, 1023, N_BIG - 1023 - 2049, 255, False), (2049, 2047, 0, 255, True), (2049, 2048, 0, 0, True)]
# (m_a, m_b, before, lo_b % 256)
TWO_CASES = [(2049, 2049, 1024, 1), (2049, 2049, 1022, 255), (2049, 2048, 1000, 3049 % 256), (2048, 2049, 1000, 3048 % 256)]
ALL_CASES = [2049, 4097]
LATTICE_N = [2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4097]
# (gw, gh, ncell + 1, tiles).  ncell + 1 = 16384, 16385, 32768, 32769 as they are.  16383 would need gw * gh = 16382 = 2 * 8191 with
# 8191 prime, so 16381 = 42 * 390 + 1 stands in for it (126 x 130 has no box side that is an exact f32 multiple of h), and
# 32767 = 258 * 127 + 1 is the table that ends one item short of a tile.  (ncell + 1) % 16 = 13, 0, 1, 15, 0, 1.
# 1032^2 + 1 items are 66 tiles (the last workgroup's look-back can take a second 64-tile trip), 1460^2 + 1 are 131 (a third).
TABLE_CASES = [(42, 390, 16381, 1), (129, 127, 16384, 1), (128, 128, 16385, 2), (258, 127, 32767, 2), (217, 151, 32768, 2),
               (256, 128, 32769, 3), (1032, 1032, 1065025, 66), (1460, 1460, 2131601, 131)]
