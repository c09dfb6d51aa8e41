"""The per-step protocol of one rank, generic over its engine (engine.SlabEngine)."""
import numpy as np

from . import partition


class SlabProtocolError(RuntimeError):
    """A device counter (lost / overflow / far_halo) is non-zero: particles were dropped or a message / the slot
    array overflowed.  The run is no longer a valid simulation of the scene."""


def _accel(tick):
    """|gravity|, the one body force."""
    return float(np.hypot(tick.gravity.x, tick.gravity.y))


class SlabDriver:
    """Per-step protocol: pack -> neighbour exchange -> finish; optional re-balancing.

    Every re-balancing step (already a host synchronisation) also (1) reads the device violation counters of
    every rank and raises SlabProtocolError if any is non-zero — a long run can no longer delete particles
    silently; (2) sizes the outer-edge margin from the largest particle speed of all ranks and the number of
    steps until the next re-trim (`travel_margin`), never below `trim_margin`; (3) shortens the interval to the
    next re-balancing step while the partition is badly unbalanced (boundaries move at most `max_shift` columns
    per step, so a rank could otherwise outgrow its slot capacity between two of them).  (2) and (3) are
    partition.plan_rebalance."""

    def __init__(self, engine, transport, bounds, grid_w, rebalance_every=0, max_shift=2, trim_margin=None,
                 capacity_main=None, check_counters=True, max_cols=None):
        self.e, self.t = engine, transport
        self.bounds = list(bounds)                 # bounds[0] / bounds[-1] are the (possibly trimmed) outer edges
        self.grid_w = grid_w
        self.rebalance_every, self.max_shift = rebalance_every, max_shift
        self.trim_margin = partition.default_trim_margin() if trim_margin is None else trim_margin
        self.capacity_main = capacity_main         # main slots per rank (None: no capacity-driven interval)
        self.check_counters = check_counters
        self.max_cols = max_cols                   # widest window the engine was created for (None: the whole grid)
        self.steps = 0
        self.next_rebalance = rebalance_every
        self.last_margin = self.trim_margin
        self.tick = None
        self.initial_vmax = 0.0                    # largest speed of the initial state (callers that start with moving particles set it)
        self.last_boundary = None

    def _set_boundary(self, cols):
        """Overlapped engines: the boundary zone for the speeds expected until the next re-balancing step."""
        self.last_boundary = cols
        self.e.set_boundary_cols(cols)

    def step(self, tick):
        self.tick = tick
        if self.steps == 0:
            self._set_boundary(partition.boundary_columns(self.initial_vmax, _accel(tick), tick.delta,
                                                          float(self.e.settings.smoothing_radius), self.rebalance_every or 64))
        self.e.pack(tick)           # overlapped engine: the pack AND everything that needs no incoming message
        self.e.exchange()
        self.e.finish()             # overlapped engine: the boundary strips
        self.steps += 1
        if self.rebalance_every and self.steps >= self.next_rebalance:
            self.rebalance()

    def rebalance(self):
        # the inputs, all-reduced.  A device-resident engine: two all-reduces, ONE host read; the torch-nccl and the
        # fs_comm_allreduce reduces (transport.reduce_rebalance) have only ever run single-rank (no multi-GPU box):
        # tests/test_multi_gpu.py compares the device path with the host path over gloo, world 2
        hist, stats = self.e.rebalance_inputs(self.grid_w)
        if not self.check_counters:
            stats[:3] = 0
        if stats[:3].any():
            raise SlabProtocolError(f"slab protocol violated at step {self.steps}: max over ranks of lost/overflow/far_halo = "
                                    f"{int(stats[0])}/{int(stats[1])}/{int(stats[2])}")
        tick = self.tick                # None before the first step: no speed-derived margin, no boundary zone
        new, interval, margin, boundary = partition.plan_rebalance(
            self.bounds, hist, stats[3], _accel(tick) if tick is not None else 0.0, tick.delta if tick is not None else None,
            float(self.e.settings.smoothing_radius), self.rebalance_every, self.max_shift, self.trim_margin,
            self.capacity_main, self.max_cols)
        self.next_rebalance = self.steps + interval
        self.last_margin = margin
        if tick is not None:
            self._set_boundary(boundary)
        if new != self.bounds:
            self.bounds = new
            self.e.set_window(new[self.t.rank], new[self.t.rank + 1])
