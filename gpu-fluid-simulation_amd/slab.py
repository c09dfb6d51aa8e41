"""One rank of the multi-GPU slab decomposition (include/fluidsim.h fs_slab_*); multi/ is its driver."""
import ctypes as C

import numpy as np

from ._abi import FS_SLAB_ROWMAJOR, FS_SLAB_SERIAL, FS_SLAB_STRIPS, PARTICLE_DTYPE, SlabConfig, SlabCounters
from ._handle import _check, _Engine, _ptr


class SlabSimulation(_Engine):
    """One rank of the multi-GPU slab decomposition (include/fluidsim.h fs_slab_*).

    Owns the global cell columns [own_lo, own_hi).  A step is pack() -> exchange the two
    messages with the slab neighbours -> step(); see multi/ for the driver.
    """
    _prefix = "fs_"
    _destroy = "fs_destroy"        # a slab is a simulation handle: made by fs_slab_create, freed by fs_destroy

    def __init__(self, settings, own_lo, own_hi, has_left, has_right, capacity, recv_capacity, max_cols, device=0,
                 sort_mode=None, serial=False, strips=False, rowmajor=False):
        super().__init__()
        self.settings = settings
        mode = (0 if sort_mode is None else 1 + int(sort_mode)) | (FS_SLAB_SERIAL if serial else 0) | (FS_SLAB_STRIPS if strips else 0)
        mode |= FS_SLAB_ROWMAJOR if rowmajor else 0        # row-major cell ids even where a slab edge has a neighbour
        self.cfg = SlabConfig(int(own_lo), int(own_hi), int(bool(has_left)), int(bool(has_right)), int(capacity),
                              int(recv_capacity), int(max_cols), mode)
        _check(self._lib, self._lib.fs_slab_create(C.byref(settings), int(device), C.byref(self.cfg), C.byref(self._h)))
        self.capacity = int(capacity)
        self.device_index = int(device)
        self.message_bytes = int(self._lib.fs_slab_message_bytes(self._h))
        # 0 serial step; 1 edge-first (default): step() advances the edge columns, builds the NEXT step's messages and only
        # then advances the interior — the exchange runs beside that on comm_stream_ptr; 2 strips: pack() also enqueues the
        # interior columns' whole step, step() the boundary strips (include/fluidsim.h)
        self.step_mode = int(self._lib.fs_slab_overlapped(self._h))
        self.overlapped = self.step_mode != 0

    def set_boundary_cols(self, cols):
        self._call("slab_set_boundary_cols", int(cols))

    @property
    def boundary_cols(self):
        return int(self._lib.fs_slab_boundary_cols(self._h))

    @property
    def comm_stream_ptr(self):
        return self._lib.fs_slab_comm_stream(self._h)

    def comm_begin(self):
        self._call("slab_comm_begin")

    def comm_end(self):
        self._call("slab_comm_end")

    def wait_packed(self):
        """Block the host until the outgoing messages of the current pack() are complete."""
        self._call("slab_wait_packed")

    def upload_owned(self, arr):
        arr = np.ascontiguousarray(arr, dtype=PARTICLE_DTYPE)
        self._call("slab_upload_owned", _ptr(arr), arr.shape[0])

    def upload_force_field(self, field):
        """As FluidSimulation.upload_force_field: f32 [texture_size.y, texture_size.x, 2]."""
        field = np.ascontiguousarray(field, dtype=np.float32)
        h, w = field.shape[0], field.shape[1]
        self._call("upload_force_field", _ptr(field), w, h)

    def set_window(self, own_lo, own_hi):
        self._call("slab_set_window", int(own_lo), int(own_hi))
        self.cfg.own_lo, self.cfg.own_hi = int(own_lo), int(own_hi)

    def pack(self, tick_settings, send_left_ptr, send_right_ptr):
        self._call("slab_pack", C.byref(tick_settings), send_left_ptr, send_right_ptr)

    def step(self, recv_left_ptr, recv_right_ptr):
        self._call("slab_step", recv_left_ptr, recv_right_ptr)

    def counters(self):
        c = SlabCounters()
        self._call("slab_counters_read", C.byref(c))
        return {"n_live": c.n_live, "lost": c.lost, "overflow": c.overflow, "far_halo": c.far_halo}

    def download(self):
        """(records with GLOBAL cell keys, owned mask) of the live slots."""
        out = np.empty(self.capacity, dtype=PARTICLE_DTYPE)
        owned = np.zeros(self.capacity, dtype=np.uint8)
        n = C.c_uint32()
        self._call("slab_download", _ptr(out), _ptr(owned), self.capacity, C.byref(n))
        return out[: n.value], owned[: n.value].astype(bool)

    def column_histogram(self, grid_w_global):
        h = np.zeros(int(grid_w_global), dtype=np.uint32)
        self._call("slab_column_histogram", _ptr(h), h.shape[0])
        return h

    def max_speed(self):
        v = C.c_float()
        self._call("slab_max_speed", C.byref(v))
        return float(v.value)

    def rebalance_stats(self, stats_dev_ptr, hist_dev_ptr, grid_w_global):
        """Enqueue the re-balancing inputs into two DEVICE buffers (4 x u32 stats, grid_w x u32 histogram); no read-back."""
        self._call("slab_rebalance_stats", stats_dev_ptr, hist_dev_ptr, int(grid_w_global))
