"""What the GPU tests of the bodies, the colliders and the 3D surface tension share when they compare a handle with the CPU
statement: the byte comparison of two record arrays (and its form for records that hold a NaN; both are tests/bitcmp.py's record
comparer), the settings' box as a tuple and the reference bodies into a handle.  TEST INFRASTRUCTURE ONLY."""
from tests.bitcmp import assert_records_equal


_same = assert_records_equal                                             # every field of every particle on its bits, `pad` aside


def _same_but_nan_bits(got, want, ctx):
    """... except that a NaN need only be a NaN: inf - inf has no defined sign or payload"""
    assert_records_equal(got, want, ctx, nan_any=True)


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
