"""Self-tests of the library that need no simulation handle: the sort on bare keys, and the sort-plan policy on the CPU."""
import ctypes as C

import numpy as np

from ._abi import load_library
from ._handle import _check, _ptr


def selftest_sort(keys, fuse_stage=-1, device=0):
    """The engine's sort (reference network, sort.wgsl:27-51) on bare u32 keys: (sorted_keys, perm, plan).

    plan = (calls that took the shifted late-stage merge, calls that took the per-stage plan); see
    csrc/kernels_sort_global.inc k_late_cert.  fuse_stage: -1 default plan, 0 per-stage only, k shifted merge from stage k.
    """
    lib = load_library()
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    pairs = (k.astype(np.uint64) << np.uint64(32)) | np.arange(k.shape[0], dtype=np.uint64)
    plan = (C.c_uint32 * 2)()
    _check(lib, lib.fs_selftest_sort(int(device), _ptr(pairs), k.shape[0], int(fuse_stage), plan))
    return (pairs >> np.uint64(32)).astype(np.uint32), (pairs & np.uint64(0xFFFFFFFF)).astype(np.uint32), (plan[0], plan[1])


def selftest_sort_policy(required, log2_count=24, start_back=8, lag=4):
    """Replay the sort-plan policy (csrc/sort_policy.h) on the CPU against a per-step `required` stage; returns
    (stage chosen per step, single stand-by launch in the stream per step).  See fs_selftest_sort_policy."""
    lib = load_library()
    req = np.ascontiguousarray(required, dtype=np.uint32)
    stage = np.zeros(req.shape[0], dtype=np.uint32)
    single = np.zeros(req.shape[0], dtype=np.uint32)
    U = C.POINTER(C.c_uint32)
    _check(lib, lib.fs_selftest_sort_policy(int(log2_count), int(start_back), int(lag), req.ctypes.data_as(U), req.shape[0],
                                            stage.ctypes.data_as(U), single.ctypes.data_as(U)))
    return stage, single
