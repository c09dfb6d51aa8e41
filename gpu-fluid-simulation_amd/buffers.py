"""Device buffers behind the C ABI: the growable one of the reference, and the consumer side of an exported range."""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import load_library
from ._handle import _check, _Handle, _ptr


class ResizableBuffer(_Handle):
    """ResizableBuffer<T> (src/buffer.rs:17-88) over HIP device memory."""
    _prefix = "fs_buffer_"
    _destroy = "fs_buffer_destroy"

    def __init__(self, name, dtype, length, device=0):
        super().__init__()
        self.dtype = np.dtype(dtype)
        st = self._lib.fs_buffer_create(int(device), self.dtype.itemsize, int(length), name.encode(), C.byref(self._h))
        _check(self._lib, st)

    def __len__(self):
        return int(self._lib.fs_buffer_len(self._h))

    def resize(self, new_cap):
        r = C.c_int()
        self._call("resize", int(new_cap), C.byref(r))
        return bool(r.value)

    def write(self, offset, data):
        data = np.ascontiguousarray(data, dtype=self.dtype)
        self._call("write", int(offset), _ptr(data), data.shape[0])

    def read(self, offset=0, count=None):
        count = len(self) - offset if count is None else count
        out = np.zeros(max(count, 0), dtype=self.dtype)
        self._call("read", int(offset), _ptr(out), out.shape[0])
        return out

    @property
    def device_ptr(self):
        return self._lib.fs_buffer_device_ptr(self._h)


class ImportedBuffer:
    """Consumer side of fs_export_handle in another process: maps the exported device range (fs_import_open)."""

    def __init__(self, handle_bytes, device=0):
        self._lib = load_library()
        self.handle = _abi.MemHandle.from_buffer_copy(handle_bytes)
        self._p = C.c_void_p()
        _check(self._lib, self._lib.fs_import_open(C.byref(self.handle), int(device), C.byref(self._p)))

    def read(self, dtype, count=None, offset=0):
        dtype = np.dtype(dtype)
        count = int(self.handle.bytes // dtype.itemsize) if count is None else int(count)
        out = np.empty(count, dtype=dtype)
        _check(self._lib, self._lib.fs_import_read(self._p, int(offset), _ptr(out), out.nbytes))
        return out

    def close(self):
        if self._p.value:
            _check(self._lib, self._lib.fs_import_close(self._p))
            self._p = C.c_void_p()
