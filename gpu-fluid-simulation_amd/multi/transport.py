"""The three ways a rank's two messages reach its slab neighbours, behind one interface (`SlabTransport`):
  * `HostTransport`     host tensors over gloo, staged through device buffers the transport owns
  * `DeviceTransport`   torch CUDA tensors over nccl (= RCCL), written and read in place by the kernels
  * `NativeTransport`   the C ABI's own RCCL binding (fs_comm_init / fs_slab_exchange), no torch on the data path
`Transport(...)` makes one of the first two, by its `device` argument."""
import ctypes as C

import numpy as np

MESSAGES = ("send_left", "send_right", "recv_left", "recv_right")


class SlabTransport:
    """What an engine and the driver ask of a transport.  rank-1 is the left neighbour, rank+1 the right one;
    `send_left`, `send_right`, `recv_left`, `recv_right` are the four messages, `torch` / `dist` the modules the tiny
    re-balancing all-reduces go through, `reduce_device` the torch device they run on (None: host tensors)."""
    INTERFACE = ("bind", "ptr", "stage_out", "stage_in", "exchange", "reduce_rebalance", "allreduce_sum", "allreduce_max")

    def __init__(self, rank, world, loopback, reduce_device):
        import torch
        import torch.distributed as dist
        self.torch, self.dist = torch, dist
        self.rank, self.world = rank, world
        self.left = rank - 1 if rank > 0 else None
        self.right = rank + 1 if rank < world - 1 else None
        if loopback:     # tests: both neighbours are this rank itself — what it sends right arrives as its right-hand incoming
            self.left = self.right = rank          # message, likewise left (sends and receives to one peer match in order)
        self.reduce_device = reduce_device
        self.g = self.sim = None
        self._reb, self._reb_gw = None, None

    def bind(self, g, sim):
        """Attach the SlabSimulation `sim` (of package `g`) whose messages this transport moves."""
        self.g, self.sim = g, sim

    def ptr(self, name):
        """Device pointer the kernels write (send_*) or read (recv_*) for message `name`: the message itself, in place."""
        return C.c_void_p(getattr(self, name).data_ptr())

    def stage_out(self):
        """After fs_slab_pack: bring the outgoing messages to where exchange() sends them from."""

    def stage_in(self):
        """Before fs_slab_step: bring the incoming messages to where ptr("recv_*") points."""

    def exchange(self):
        """The neighbour exchange of one step."""
        raise NotImplementedError

    def reduce_rebalance(self, gw):
        """fs_slab_rebalance_stats of the bound simulation, reduced over all ranks and read ONCE: uint32[gw + 4] on the
        host = the column histogram (SUM), then lost, overflow, far_halo and the bits of the largest speed (MAX)."""
        raise NotImplementedError

    def _rebalance_buffer(self, gw):
        """The fs_buffer the gw + 4 words are produced into, and its device address."""
        if self._reb_gw != gw:
            self._reb = self.g.ResizableBuffer("rebalance", np.uint32, gw + 4, device=self.sim.device_index)
            self._reb_gw = gw
        base = self._reb.device_ptr
        self.sim.rebalance_stats(C.c_void_p(base + 4 * gw), C.c_void_p(base), gw)
        return base

    def _allreduce(self, arr, op):
        th = self.torch.from_numpy(arr)
        if self.reduce_device is not None:
            th = th.to(self.reduce_device)
        self.dist.all_reduce(th, op=op)
        return th.cpu().numpy()

    def allreduce_sum(self, arr):
        """A host array summed over all ranks (tiny, every K steps only)."""
        return self._allreduce(arr, self.dist.ReduceOp.SUM)

    def allreduce_max(self, arr):
        return self._allreduce(arr, self.dist.ReduceOp.MAX)


class _TorchP2P(SlabTransport):
    """The messages are torch tensors, exchanged with torch.distributed's batched isend / irecv."""

    def __init__(self, rank, world, message_bytes, device, loopback):
        super().__init__(rank, world, loopback, device)
        torch, dist = self.torch, self.dist
        kw = {"dtype": torch.uint8, "device": device} if device is not None else {"dtype": torch.uint8}
        self.send_left = torch.zeros(message_bytes, **kw)
        self.send_right = torch.zeros(message_bytes, **kw)
        self.recv_left = torch.zeros(message_bytes, **kw)
        self.recv_right = torch.zeros(message_bytes, **kw)
        # the four descriptors never change (fixed tensors, fixed peers): build them once
        self.ops = []
        if self.right is not None:
            self.ops.append(dist.P2POp(dist.isend, self.send_right, self.right))
            self.ops.append(dist.P2POp(dist.irecv, self.recv_right, self.right))
        if self.left is not None:
            self.ops.append(dist.P2POp(dist.isend, self.send_left, self.left))
            self.ops.append(dist.P2POp(dist.irecv, self.recv_left, self.left))

    def exchange(self):
        if not self.ops:
            return
        for req in self.dist.batch_isend_irecv(self.ops):
            req.wait()          # nccl: makes the current stream wait; gloo: blocks the host


class HostTransport(_TorchP2P):
    """Host tensors (gloo).  Bound to a SlabSimulation, it owns the four device buffers the kernels write and read and
    copies between them and the host tensors around the exchange."""

    def __init__(self, rank, world, message_bytes, loopback=False):
        super().__init__(rank, world, message_bytes, None, loopback)
        self.dev = None

    def bind(self, g, sim):
        super().bind(g, sim)
        self.dev = {k: g.ResizableBuffer(k, np.uint8, sim.message_bytes, device=sim.device_index) for k in MESSAGES}

    def ptr(self, name):
        return C.c_void_p(self.dev[name].device_ptr)

    def stage_out(self):
        self.sim.wait_packed()      # the messages only: an overlapped handle goes on computing its interior columns
        self.send_left.numpy()[:] = self.dev["send_left"].read()
        self.send_right.numpy()[:] = self.dev["send_right"].read()

    def stage_in(self):
        self.dev["recv_left"].write(0, self.recv_left.numpy())
        self.dev["recv_right"].write(0, self.recv_right.numpy())

    def reduce_rebalance(self, gw):
        """One device read, then the all-reduces on the host."""
        self._rebalance_buffer(gw)
        self.sim.sync()
        host = self._reb.read()
        th, ts = self.torch.from_numpy(host[:gw].astype(np.int64)), self.torch.from_numpy(host[gw:].astype(np.int64))
        self.dist.all_reduce(th, op=self.dist.ReduceOp.SUM)
        self.dist.all_reduce(ts, op=self.dist.ReduceOp.MAX)
        return np.concatenate([th.numpy(), ts.numpy()]).astype(np.uint32)


class DeviceTransport(_TorchP2P):
    """Torch CUDA tensors (nccl = RCCL over xGMI).  The caller makes the simulation's stream torch's current stream, so
    RCCL orders after the pack and before the unpack; bound to an overlapped handle, the exchange is issued on the
    handle's exchange stream instead (behind the pack, beside the interior columns' kernels; fs_slab_step waits for it)."""

    def __init__(self, rank, world, message_bytes, device, loopback=False):
        super().__init__(rank, world, message_bytes, device, loopback)
        self.device = device
        self._comm_ext = None

    def bind(self, g, sim):
        super().bind(g, sim)
        if sim.overlapped and self.ops:
            self._comm_ext = self.torch.cuda.ExternalStream(sim.comm_stream_ptr, device=self.device)

    def exchange(self):
        if self._comm_ext is None:      # a serial handle, or no neighbour
            super().exchange()
            return
        self.sim.comm_begin()
        with self.torch.cuda.stream(self._comm_ext):
            super().exchange()
        self.sim.comm_end()

    def reduce_rebalance(self, gw):
        """torch.distributed on the device buffer, then ONE read."""
        if self._reb_gw != gw:
            self._reb = self.torch.zeros(gw + 4, dtype=self.torch.int32, device=self.device)
            self._reb_gw = gw
        base = self._reb.data_ptr()
        self.sim.rebalance_stats(C.c_void_p(base + 4 * gw), C.c_void_p(base), gw)
        self.sim.sync()                        # produced on the simulation's stream, which need not be torch's current one
        self.dist.all_reduce(self._reb[:gw], op=self.dist.ReduceOp.SUM)
        self.dist.all_reduce(self._reb[gw:], op=self.dist.ReduceOp.MAX)
        return self._reb.cpu().numpy().view(np.uint32)


def Transport(rank, world, message_bytes, device=None, loopback=False):
    """Exchange one byte message with each slab neighbour through torch.distributed: `device` is torch.device("cuda", i)
    for nccl, None for host tensors (gloo)."""
    if device is None:
        return HostTransport(rank, world, message_bytes, loopback)
    return DeviceTransport(rank, world, message_bytes, device, loopback)


class _DevMsg:
    """A device message buffer with the accessor of a torch tensor that a transport's ptr() needs."""

    def __init__(self, g, name, nbytes, device_index):
        self.buf = g.ResizableBuffer(name, np.uint8, nbytes, device=device_index)

    def data_ptr(self):
        return self.buf.device_ptr


class NativeTransport(SlabTransport):
    """The same neighbour exchange through the C ABI's own RCCL binding (fs_comm_init / fs_slab_exchange,
    csrc/comm.hip): grouped ncclSend/ncclRecv on the simulation's stream (fs_slab_exchange does the hand-over to an
    overlapped handle's exchange stream itself), no torch tensor or torch stream on the data path — what a Rust (or any
    non-Python) host calls.  torch.distributed is used ONCE, to ship rank 0's 128-byte RCCL id to the other ranks; any
    rendezvous would do.  Opt-in: FS_NATIVE_RCCL=1 for bench.py --gpus N.
    `reduce_device`: where the host path's all-reduces (FS_REBALANCE_HOST, tiny, every K steps) run on torch."""

    def __init__(self, g, rank, world, message_bytes, device_index, dist=None, loopback=False, reduce_device=None):
        super().__init__(rank, world, loopback, reduce_device)
        self.g = g
        self.send_left, self.send_right, self.recv_left, self.recv_right = (
            _DevMsg(g, k, message_bytes, device_index) for k in MESSAGES)
        lib = g.load_library()
        idbuf = (C.c_uint8 * 128)()
        if rank == 0:
            g._check(lib, lib.fs_comm_unique_id(idbuf))
        if world > 1:
            box = [bytes(idbuf)]
            dist.broadcast_object_list(box, src=0)
            idbuf = (C.c_uint8 * 128).from_buffer_copy(box[0])
        self.comm = C.c_void_p()
        g._check(lib, lib.fs_comm_init(int(device_index), rank, world, idbuf, C.byref(self.comm)))
        self.lib = lib

    def exchange(self):
        self.g._check(self.lib, self.lib.fs_slab_exchange(
            self.sim._h, self.comm, -1 if self.left is None else self.left, -1 if self.right is None else self.right,
            self.ptr("send_left"), self.ptr("send_right"), self.ptr("recv_left"), self.ptr("recv_right")))

    def reduce_rebalance(self, gw):
        """fs_comm_allreduce on the simulation's stream, then ONE read."""
        g, lib, h = self.g, self.lib, self.sim._h
        base = self._rebalance_buffer(gw)
        g._check(lib, lib.fs_comm_allreduce(h, self.comm, C.c_void_p(base), gw, 0, 0))              # u32, SUM
        g._check(lib, lib.fs_comm_allreduce(h, self.comm, C.c_void_p(base + 4 * gw), 4, 0, 1))       # u32, MAX
        self.sim.sync()                        # the ONE host synchronisation of a re-balancing step
        return self._reb.read()

    def close(self):
        if self.comm.value:
            self.lib.fs_comm_destroy(self.comm)
            self.comm = C.c_void_p()
