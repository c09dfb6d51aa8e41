"""Which status a device ordinal outside [0, ndev) maps to, per entry point that takes one.  The create calls say
FS_ERR_INVALID (a bad argument of a handle that does not exist yet); the calls that work without a handle say FS_ERR_DEVICE.
Nothing here launches a kernel: every call below returns from its device check."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAD_ORDINALS = (-1, 4096)


def _calls(fs, lib):
    """name -> (expected status, callable(device) -> status); the out-pointers every call writes are checked by the caller."""
    abi = fs._abi
    st2, _, _ = fs.dam_break_2d(4096)
    st3, _, _ = fs.dam_break_3d(4096)
    image = np.zeros((4, 4), dtype=np.uint8)
    pairs = np.arange(8, dtype=np.uint64)
    handle = abi.MemHandle()      # zeroed
    out = C.c_void_p()
    bad = C.c_uint32(0)

    def create(dev):
        return lib.fs_create(C.byref(st2), dev, C.byref(out))

    def create3(dev):
        return lib.fs3_create(C.byref(st3), dev, abi.Vec3(0.0, 0.0, 0.0), C.byref(out))

    def constdiv(dev):
        return lib.fs_selftest_constdiv(dev, C.c_float(0.04), C.c_float(25.0), C.c_float(2.0 ** -60), C.c_float(0.04), C.byref(bad))

    def sort(dev):
        return lib.fs_selftest_sort(dev, pairs.ctypes.data_as(C.c_void_p), 8, -1, None)

    def field(dev):
        return lib.fs_generate_force_field(None, dev, image.ctypes.data_as(C.c_void_p), 4, 4, None)

    def import_open(dev):
        return lib.fs_import_open(C.byref(handle), dev, C.byref(out))

    return out, {
        "fs_create": (abi.FS_ERR_INVALID, create),
        "fs3_create": (abi.FS_ERR_INVALID, create3),
        "fs_selftest_constdiv": (abi.FS_ERR_DEVICE, constdiv),
        "fs_selftest_sort": (abi.FS_ERR_DEVICE, sort),
        "fs_generate_force_field": (abi.FS_ERR_DEVICE, field),
        "fs_import_open": (abi.FS_ERR_DEVICE, import_open),
    }


def test_out_of_range_device_ordinals(fs):
    lib = fs.load_library()
    abi = fs._abi
    out, calls = _calls(fs, lib)
    for name, (want, call) in calls.items():
        for dev in BAD_ORDINALS:
            # a message of another kind first, so that "non-empty" below is about this call
            assert lib.fs_grid_dims(None, None, None) == abi.FS_ERR_INVALID and lib.fs_last_error() == b"null argument"
            got = call(dev)
            msg = lib.fs_last_error()
            print(f"{name}(device={dev}): status {got}, {msg!r}")
            assert got == want, f"{name}(device={dev}): status {got}, expected {want} ({msg!r})"
            assert msg and msg != b"null argument", f"{name}(device={dev}) left no message of its own"
            assert not out.value, f"{name}(device={dev}) handed out a handle / pointer"

    # ... and none of it leaves the process in a state a valid create cannot start from
    st, _, tick = fs.dam_break_2d(4096)
    sim = C.c_void_p()
    assert lib.fs_create(C.byref(st), 0, C.byref(sim)) == abi.FS_OK, lib.fs_last_error()
    try:
        assert lib.fs_step(sim, C.byref(tick)) == abi.FS_OK, lib.fs_last_error()
        rec = np.zeros(4096, dtype=fs.PARTICLE_DTYPE)
        assert lib.fs_download_particles(sim, rec.ctypes.data_as(C.c_void_p), rec.shape[0]) == abi.FS_OK, lib.fs_last_error()
        assert lib.fs_tick_count(sim) == 1
        assert np.isfinite(rec["position"]).all() and (rec["density"] > 0).all()
    finally:
        lib.fs_destroy(sim)
