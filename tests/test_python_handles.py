"""The life cycle that the Python wrapper's handle base owns (gpu-fluid-simulation_amd/_handle.py): close() is safe on an
object whose __init__ never ran, it is idempotent, and every handle class frees its handle through its own destroy call.  The
slab is the case that matters: it is made by fs_slab_create and freed by fs_destroy, which no prefix rule gives.  No GPU."""
import collections
import ctypes as C

import pytest

# class -> the one call of the library that frees its handle
DESTROY = {"FluidSimulation": "fs_destroy", "FluidSimulation3D": "fs3_destroy", "SlabSimulation": "fs_destroy",
           "ResizableBuffer": "fs_buffer_destroy"}


class CountingLib:
    """Stand-in for the library: every attribute is a call that succeeds; calls are counted per name."""

    def __init__(self):
        self.calls = collections.Counter()

    def __getattr__(self, name):
        def call(*args):
            self.calls[name] += 1
            return 0
        return call


@pytest.mark.parametrize("cls_name", sorted(DESTROY))
def test_close_survives_a_half_constructed_object(fs, cls_name):
    obj = object.__new__(getattr(fs, cls_name))
    assert not hasattr(obj, "_h") and not hasattr(obj, "_lib")
    obj.close()
    obj.close()
    obj.__del__()


@pytest.mark.parametrize("cls_name", sorted(DESTROY))
def test_close_destroys_once_through_the_class_own_call(fs, cls_name):
    obj = object.__new__(getattr(fs, cls_name))
    obj._lib = CountingLib()
    obj._h = C.c_void_p(1)
    obj.close()
    obj.close()
    assert dict(obj._lib.calls) == {DESTROY[cls_name]: 1}
    assert not obj._h.value
    obj.__del__()
    assert dict(obj._lib.calls) == {DESTROY[cls_name]: 1}
