"""Everything of the slab driver that needs only numpy: the message layout, the column partition, its re-balancing
policy and the sizes of a rank's slot array."""
import os

import numpy as np

HEADER_BYTES = 16
RECORD_BYTES = 16


def global_columns(positions_x, bounds_x, h):
    """Global cell column of x (funcs.wgsl:212-214) in f32, for host-side partitioning."""
    f = np.float32
    c = np.floor((positions_x.astype(f) + f(bounds_x) * f(0.5)) / f(h))
    return np.clip(c, 0, 4294967295.0).astype(np.int64) + 1


def partition_columns(hist, world, min_cols=4):
    """Boundaries b[0..world] (b[0]=0, b[world]=len(hist)) giving ~equal particle counts."""
    gw = len(hist)
    csum = np.concatenate([[0], np.cumsum(hist.astype(np.int64))])
    total = csum[-1]
    b = [0]
    for r in range(1, world):
        target = total * r // world
        c = int(np.searchsorted(csum, target, side="left"))
        c = max(c, b[-1] + min_cols)
        c = min(c, gw - (world - r) * min_cols)
        b.append(c)
    b.append(gw)
    return b


def rebalance_boundaries(bounds, hist, max_shift, min_cols=4):
    """Move each interior boundary towards the equal-count partition by at most max_shift columns."""
    world = len(bounds) - 1
    ideal = partition_columns(hist, world, min_cols)
    new = list(bounds)
    for k in range(1, world):
        d = int(np.clip(ideal[k] - bounds[k], -max_shift, max_shift))
        new[k] = bounds[k] + d
    for k in range(1, world):                      # keep slabs at least min_cols wide
        new[k] = max(new[k], new[k - 1] + min_cols)
    for k in range(world - 1, 0, -1):
        new[k] = min(new[k], new[k + 1] - min_cols)
    return new


def trim_outer_edges(bounds, hist, margin, min_cols=4):
    """The first and last slab own everything out to the domain walls, which in a dam break is mostly empty
    space: their local grids (and with them the cell-start table and the counting sort's scan) would be many
    times larger than an inner slab's, and the slowest rank sets the pace.  Pull the two OUTER edges in to
    `margin` columns beyond the occupied columns (never past the walls, never inside a neighbour).  A particle
    that outruns the margin between two re-balancing steps is counted as `lost` by the slab engine, like any
    other protocol violation.  margin <= 0 keeps the walls."""
    gw = len(hist)
    new = list(bounds)
    occ = np.nonzero(np.asarray(hist))[0]
    if margin <= 0 or occ.size == 0:
        new[0], new[-1] = 0, gw
        return new
    new[0] = int(min(max(0, int(occ[0]) - margin), new[1] - min_cols))
    new[-1] = int(max(min(gw, int(occ[-1]) + 1 + margin), new[-2] + min_cols))
    return new


def default_trim_margin():
    """Floor of the outer-edge margin in columns (FS_SLAB_TRIM_MARGIN); the margin actually used is
    max(this, travel_margin(...)) so that it is tied to how far the fluid can move before the next re-trim."""
    return int(os.environ.get("FS_SLAB_TRIM_MARGIN", "256"))


SPEED_CLAMP = 500.0          # compute.wgsl:118-122: |v| <= 500 after every step


def boundary_columns(vmax, accel, dt, h, steps, safety=1.5, floor=4):
    """Width of the boundary zone of an overlapped slab step (fs_slab_set_boundary_cols): a migrant must land at least 3
    columns short of the interior, so 3 + the columns the fastest particle can cross in ONE step at any time before the next
    re-balancing step (`steps` steps away; vmax = largest speed now, all ranks).  Never below `floor`."""
    v_end = min(SPEED_CLAMP, safety * float(vmax) + float(accel) * float(dt) * steps)
    return max(int(floor), 3 + int(np.ceil(v_end * float(dt) / float(h))))


def travel_margin(vmax, accel, dt, h, steps, safety=1.5):
    """Columns a particle can cross in `steps` steps: it moves at most (safety * vmax + accel * dt * k) * dt in
    step k (vmax = largest speed now, all ranks; accel = |gravity|, the one body force; `safety` covers pressure
    pushes), never faster than the engine's speed clamp.  +2: the slab's own 2-column halo tolerance."""
    v_end = min(SPEED_CLAMP, safety * float(vmax) + float(accel) * float(dt) * steps)
    v_mean = min(SPEED_CLAMP, 0.5 * (safety * float(vmax) + v_end))
    return int(np.ceil(steps * v_mean * float(dt) / float(h))) + 2


def plan_rebalance(bounds, hist, vmax, accel, dt, h, rebalance_every, max_shift, trim_margin, capacity_main=None,
                   max_cols=None):
    """The boundary policy of a re-balancing step: (new_bounds, interval, margin, boundary_cols) from the all-reduced
    column histogram and largest speed.
      interval       steps to the next re-balancing step: `rebalance_every`, an eighth of it while the fullest rank is past
                     90 % of `capacity_main` (without one: 15 % over the mean), half of it while it is 10 % over the mean —
                     boundaries move at most `max_shift` columns per re-balancing step, so a rank could otherwise outgrow its
                     slots between two of them
      margin         outer-edge margin in columns: `trim_margin`, or what the fastest particle can cross in `interval` steps
                     (travel_margin) if that is more
      boundary_cols  boundary zone of an overlapped step for the same interval (boundary_columns)
      new_bounds     interior boundaries moved towards equal counts, outer edges `margin` beyond the occupied columns, the
                     outer slabs never wider than `max_cols`
    dt None (no step taken yet, so no tick to take dt and the body force from): the margin stays `trim_margin` and
    boundary_cols is None."""
    world = len(bounds) - 1
    owned = np.array([hist[bounds[k]:bounds[k + 1]].sum() for k in range(world)], dtype=np.float64)
    interval = rebalance_every
    if owned.sum() > 0:
        worst = owned.max()
        limit = 0.9 * capacity_main if capacity_main else 1.15 * owned.mean()
        if worst > limit:                     # catching up: boundaries move <= max_shift columns per re-balancing step
            interval = max(1, rebalance_every // 8)
        elif worst > 1.10 * owned.mean():
            interval = max(1, rebalance_every // 2)
    new = rebalance_boundaries(bounds, hist, max_shift)
    margin, boundary = trim_margin, None
    if dt is not None:
        if margin > 0:
            margin = max(margin, travel_margin(vmax, accel, dt, h, interval))
        boundary = boundary_columns(vmax, accel, dt, h, interval)
    new = trim_outer_edges(new, hist, margin)               # outer edges follow the occupied columns
    if max_cols:                                            # never wider than the engine's tables
        new[0] = max(new[0], new[1] - max_cols)
        new[-1] = min(new[-1], new[-2] + max_cols)
    return new, interval, margin, boundary


def slab_capacities(n_total, world, grid_h, headroom=1.25):
    """(capacity, recv_capacity).  A message carries 2 ghost columns + migrants: ~2 * grid_h * 4 records at
    lattice density; 3 * grid_h * 8 leaves ~3x headroom (the device counters flag an overflow).  Smaller
    messages matter: they are sent at full size every step (no host sync to learn the real count).
    Main slots hold the worst-case owned share (mean * headroom — SlabDriver re-balances more often once a rank
    passes 90 % of it) plus the 4 ghost columns that are live after a step (2 per side, 10 particles per cell)."""
    recv = max(4096, 3 * grid_h * 8)
    main = int(n_total / world * headroom) + 4 * grid_h * 10 + 4096
    return main + 2 * recv, recv


def main_slots(capacity, recv_capacity):
    return capacity - 2 * recv_capacity


def initial_owned(g, settings, offset, bounds, rank):
    """This rank's share of the reference lattice (src/simulation.rs:147-163) + column histogram."""
    lat = g.reference_lattice(settings, offset)
    cols = global_columns(lat["position"][:, 0], settings.size.x, settings.smoothing_radius)
    lo, hi = bounds[rank], bounds[rank + 1]
    return lat[(cols >= lo) & (cols < hi)]


def lattice_histogram(g, settings, offset):
    lat = g.reference_lattice(settings, offset)
    cols = global_columns(lat["position"][:, 0], settings.size.x, settings.smoothing_radius)
    gw = int(np.ceil(np.float32(settings.size.x) / np.float32(settings.smoothing_radius))) + 2
    return np.bincount(cols, minlength=gw)[:gw].astype(np.int64), gw
