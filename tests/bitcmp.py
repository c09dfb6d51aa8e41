"""What "bit-equal" means in the tests, once: the word view, the record comparer, the byte comparison of query records, the
comparison of ids and channels, and the special-value channel contents the GPU tests upload.  TEST INFRASTRUCTURE ONLY; no
pytest mark, so CPU and GPU tests alike import it.  tests/test_support.py pins the strictness of every comparer here."""
import numpy as np
import pytest

# NaN payloads, -0.0, denormals, infinities and ordinary values ...
POOL_NINE = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0x3F800000, 0xC2F6E979],
                     dtype=np.uint32)
# ... and with a negative signalling NaN, -inf and +0.0
POOL_TWELVE = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFF8ABCDE, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000,
                        0xFF800000, 0x3F800000, 0x00000000, 0xC2F6E979], dtype=np.uint32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_words(got, want):
    """bit for bit, a NaN of `want` met by any NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


def assert_records_equal(got, want, ctx, nan_any=False):
    """Two structured arrays: the same length, and every named field of `want` the same on its bits in every entry (`pad`, which
    the 3D records carry, is the one field not compared).  nan_any: in f32 fields a NaN need only be a NaN (inf - inf has no
    defined sign or payload)."""
    assert got.shape == want.shape, f"{ctx}: {got.shape[0]} entries, expected {want.shape[0]}"
    for name in want.dtype.names:
        if name == "pad":
            continue
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        same = bits(a) == bits(b)
        if nan_any and a.dtype == np.float32:
            same |= np.isnan(a) & np.isnan(b)
        bad = ~same.all(axis=tuple(range(1, same.ndim)))
        if bad.any():
            k = int(np.argmax(bad))
            with np.errstate(all="ignore"):
                err = np.nanmax(np.abs(a[bad].astype(np.float64) - b[bad].astype(np.float64)))
            raise AssertionError(f"{ctx}: {name} not bit-exact in {int(bad.sum())} of {bad.size} entries; first {k}: "
                                 f"{a[k]} vs {b[k]}; max abs err {err:g}")


def assert_identical(got, want, what):
    """Two arrays of query records: the same shape and dtype, then the same bytes."""
    assert got.shape == want.shape, f"{what}: shape {got.shape}, expected {want.shape}"
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype}, expected {want.dtype}"
    if got.tobytes() != want.tobytes():
        g, w = got.ravel(), want.ravel()
        bad = np.flatnonzero([a.tobytes() != b.tobytes() for a, b in zip(g, w)])
        k = bad[0]
        raise AssertionError(f"{what}: {bad.size} of {g.size} records differ; first {k}: {g[k]} != {w[k]}")


def assert_track_equal(sim, chk, ctx, nan_any=False):
    """The handle's ids, channel count and every channel on its bits against a checker's ids, channels and attr."""
    got = sim.particle_ids()
    assert np.array_equal(got, chk.ids), f"{ctx}: ids differ in {int((got != chk.ids).sum())} slots"
    assert sim.track_channels == chk.channels, f"{ctx}: {sim.track_channels} channels, expected {chk.channels}"
    for c in range(chk.channels):
        a, b = sim.attribute(c), chk.attr[c]
        ok = same_words(a, b) if nan_any else bits(a) == bits(b)
        assert np.all(ok), f"{ctx}: channel {c} not bit-exact ({int(np.sum(~ok))} words differ)"


def special_bits(n, seed, pool):
    """`n` f32 words drawn from a pool of special values, mixed."""
    return pool[np.random.default_rng(seed).integers(0, pool.size, size=n)].view(np.float32)


def set_channels(sim, chk, seed):
    """special values into every channel of the handle and of its checker: seed + c for channel c, from the nine-value pool"""
    for c in range(chk.channels):
        v = special_bits(chk.n, seed + c, POOL_NINE)
        sim.set_attribute(c, v)
        chk.attr[c] = v


def expect_invalid(fs, call):
    with pytest.raises(fs.FluidSimError) as e:
        call()
    assert e.value.status == fs._abi.FS_ERR_INVALID, e.value
