"""What `SlabDriver` asks of one rank's engine (`SlabEngine`), and the engine over the C ABI (`HipSlabEngine`)."""
import os

import numpy as np


class SlabEngine:
    """One rank's local step, as the driver sees it.  `self.t` is the rank's transport (transport.SlabTransport), whose
    messages pack() fills and finish() consumes."""
    INTERFACE = ("pack", "exchange", "finish", "set_window", "set_boundary_cols", "owned_particles", "counters", "max_speed",
                 "column_histogram", "settings", "sync", "rebalance_inputs")
    t = None
    settings = None         # the scene's SimulationSettings (an attribute or a property)

    def pack(self, tick):
        """Start step `tick`: fill the outgoing messages (an overlapped engine: and everything that needs no incoming one)."""
        raise NotImplementedError

    def exchange(self):
        """The neighbour exchange of this step."""
        self.t.exchange()

    def finish(self):
        """Consume the incoming messages and complete the step."""
        raise NotImplementedError

    def set_window(self, lo, hi):
        """Own the global columns [lo, hi) from the next step on."""
        raise NotImplementedError

    def set_boundary_cols(self, cols):
        """Overlapped engines: width of the boundary zone that waits for the incoming messages."""

    def owned_particles(self):
        raise NotImplementedError

    def counters(self):
        """This rank's protocol violations so far: {"lost", "overflow", "far_halo"} (and what else the engine counts)."""
        raise NotImplementedError

    def max_speed(self):
        raise NotImplementedError

    def column_histogram(self, gw):
        """Owned particles per global column, gw columns."""
        raise NotImplementedError

    def sync(self):
        raise NotImplementedError

    def rebalance_inputs(self, gw):
        """(column histogram summed over ranks as int64[gw], [lost, overflow, far_halo, vmax] maxed over ranks as
        float64[4]).  Here: three blocking reads, then two tiny all-reduces of host arrays through the transport's torch
        process group."""
        hist = self.t.allreduce_sum(self.column_histogram(gw).astype(np.int64))
        c = self.counters()
        stats = np.array([c["lost"], c["overflow"], c["far_halo"], float(self.max_speed())], dtype=np.float64)
        return hist, self.t.allreduce_max(stats)


class HipSlabEngine(SlabEngine):
    """Adapter over the C ABI (`fs_slab_*`).  The kernels write and read the messages where the transport says
    (transport.ptr): in place with a device transport, in the host transport's staging buffers otherwise."""

    def __init__(self, g, settings, bounds, rank, world, capacity, recv_capacity, max_cols, device_index, transport, **sim_kw):
        self.g = g
        self.sim = g.SlabSimulation(settings, bounds[rank], bounds[rank + 1], transport.left is not None, transport.right is not None,
                                    capacity, recv_capacity, max_cols, device=device_index, **sim_kw)
        self.t = transport
        transport.bind(g, self.sim)

    @property
    def message_bytes(self):
        return self.sim.message_bytes

    @property
    def settings(self):
        return self.sim.settings

    def pack(self, tick):
        self.sim.pack(tick, self.t.ptr("send_left"), self.t.ptr("send_right"))
        self.t.stage_out()

    def set_boundary_cols(self, cols):
        if self.sim.overlapped:
            self.sim.set_boundary_cols(cols)

    def finish(self):
        self.t.stage_in()
        self.sim.step(self.t.ptr("recv_left"), self.t.ptr("recv_right"))

    def set_window(self, lo, hi):
        self.sim.set_window(lo, hi)

    def column_histogram(self, gw):
        return self.sim.column_histogram(gw)

    def owned_particles(self):
        rec, owned = self.sim.download()
        return rec[owned]

    def counters(self):
        return self.sim.counters()

    def max_speed(self):
        return self.sim.max_speed()

    def rebalance_inputs(self, gw):
        """With ONE device read: fs_slab_rebalance_stats leaves the gw + 4 words on the device, the transport reduces them
        there (transport.reduce_rebalance) and the host reads the reduced buffer once.  FS_REBALANCE_HOST=1 keeps the
        older path of the base class."""
        if os.environ.get("FS_REBALANCE_HOST"):
            return super().rebalance_inputs(gw)
        host = self.t.reduce_rebalance(gw)
        stats = np.array([host[gw], host[gw + 1], host[gw + 2],
                          float(np.array([host[gw + 3]], dtype=np.uint32).view(np.float32)[0])], dtype=np.float64)
        return host[:gw].astype(np.int64), stats

    def sync(self):
        self.sim.sync()
