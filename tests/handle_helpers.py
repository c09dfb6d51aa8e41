"""What the GPU tests of the bodies, the colliders and the 3D surface tension share when they compare a handle with the CPU
statement: the byte comparison of two record arrays (and its form for records that hold a NaN), the settings' box as a tuple and
the reference bodies into a handle.  TEST INFRASTRUCTURE ONLY."""
import numpy as np


def _same(got, want, ctx):
    """every field of every particle, byte for byte (`pad`, which the 3D records carry, is the one field not compared)"""
    assert got.shape == want.shape, f"{ctx}: {got.shape[0]} particles, expected {want.shape[0]}"
    for name in want.dtype.names:
        if name == "pad":
            continue
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        bad = a.view(np.uint32).reshape(a.shape[0], -1) != b.view(np.uint32).reshape(b.shape[0], -1)
        assert not bad.any(), f"{ctx}: {name} differs in {int(bad.any(axis=1).sum())} particles, first {int(np.argmax(bad.any(axis=1)))}"


def _same_but_nan_bits(got, want, ctx):
    """every field on its bits (`pad` aside), except that a NaN need only be a NaN: inf - inf has no defined sign or payload"""
    assert got.shape == want.shape, f"{ctx}: {got.shape[0]} particles, expected {want.shape[0]}"
    for name in want.dtype.names:
        if name == "pad":
            continue
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        same = a.view(np.uint32) == b.view(np.uint32)
        if a.dtype == np.float32:
            same |= np.isnan(a) & np.isnan(b)
        assert same.all(), f"{ctx}: {name} differs in {int((~same).sum())} values"


def _size(st):
    """the box of 2D or 3D settings: (x, y) or (x, y, z)"""
    return tuple(getattr(st.size, a) for a in "xyz" if hasattr(st.size, a))


def _add(sim, bodies):
    """the reference bodies into a handle, in order; returns the slots"""
    slots = []
    for b in bodies:
        k = sim.add_body(b.field, b.extent)
        sim.set_body_motion(k, *b.motion())
        slots.append(k)
    return slots
