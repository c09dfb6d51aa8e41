"""The tests' own support code, held to what the other test modules rely on (no GPU): the oracle's flags in oracle/oracle.py are
the Makefile's, tests/checker_lib.py builds once per content and hands every checker the oracle's prototypes, the special-value
channel contents are the ones the tracking and emission tests have always uploaded, and the comparers of tests/bitcmp.py are as
strict as their names say."""
import hashlib
import os
import shutil

import numpy as np
import pytest

from oracle import oracle as O
from tests import bitcmp as B
from tests import checker_lib as CL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT_FIELDS = ("position", "predicted_position", "velocity", "density")
DTYPES = {"2d": O.PARTICLE_DTYPE, "3d": O.PARTICLE3_DTYPE}


# ---- 1. flags ---------------------------------------------------------------------------------------------------------------------
def test_oracle_flags_are_the_makefiles():
    with open(os.path.join(ROOT, "oracle", "Makefile")) as fh:
        lines = [ln for ln in fh if ln.startswith("CXXFLAGS ?=")]
    assert len(lines) == 1
    assert O.FLAGS == [w for w in lines[0].split("?=", 1)[1].split() if not w.startswith("-W")]
    assert CL.FLAGS == O.FLAGS + ["-shared"]


def test_no_python_file_under_tests_spells_a_flag():
    """The checkers' .cpp sources name the flag in the comment that says how they are to be built; no Python file, which is
    where a build could be spelled, does."""
    needle = "-ffp-" + "contract"
    here = os.path.join(ROOT, "tests")
    hits = []
    for d, _, names in os.walk(here):
        for name in names:
            if name.endswith(".py"):
                with open(os.path.join(d, name), errors="replace") as fh:
                    if needle in fh.read():
                        hits.append(os.path.relpath(os.path.join(d, name), here))
    assert not hits, hits


# ---- 2. the loader ------------------------------------------------------------------------------------------------------------------
def test_build_is_keyed_by_content(tmp_path):
    from tests import st_ref
    first = CL.build("st_checker", st_ref.SOURCES)
    stamp = os.stat(first).st_mtime_ns
    assert CL.build("st_checker", st_ref.SOURCES) == first and os.stat(first).st_mtime_ns == stamp, "built twice"
    assert os.path.dirname(first) == CL.cache_dir() and os.path.basename(first).startswith("libst_checker_")
    edited = tmp_path / "st_checker.cpp"
    shutil.copy(st_ref.SOURCES[0], edited)
    with open(edited, "a") as fh:
        fh.write("// edited\n")
    for sources in ([str(edited)] + st_ref.SOURCES[1:], st_ref.SOURCES[:1] + [str(edited)] + st_ref.SOURCES[2:]):
        other = CL.path_of("st_checker", sources)          # the translation unit, then something it includes
        assert other != first and os.path.dirname(other) == os.path.dirname(first)
    assert CL.path_of("st3d_checker", st_ref.SOURCES) != first


@pytest.mark.parametrize("module,family", [("st_ref", "orc_"), ("sample_ref", "orc_"), ("diffuse_ref", "orc_"), ("st3d_ref", "orc3_"),
                                           ("sample3d_ref", "orc3_"), ("render3d_ref", "orc3_"), ("mesh3d_ref", "orc3_")])
def test_a_checker_has_the_oracles_prototypes(module, family):
    import importlib
    ref = importlib.import_module(f"tests.{module}")
    L = ref.lib()
    assert ref.lib() is L, "loaded twice"
    names = [n for n in O.lib().__dict__ if n.startswith(family)]
    assert len(names) >= 8 and ("orc_sort_stable" in names) == (family == "orc_")
    for name in names:
        f, g = getattr(O.lib(), name), L.__dict__[name]
        assert g.argtypes == f.argtypes and g.restype == f.restype, name
    assert not [n for n in L.__dict__ if n.startswith("orc") and not n.startswith(family)], "a prototype of the other family"
    for name, (restype, argtypes) in ref.OWN.items():
        assert L.__dict__[name].argtypes == argtypes and L.__dict__[name].restype == restype, name


# ---- 3. the inputs did not move -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool,seed,digest", [(B.POOL_NINE, 11, "cca759a9b0acc6d4"), (B.POOL_TWELVE, 99, "193ffaafc2be4db4"),
                                              (B.POOL_TWELVE, 50, "c6fb7956de07ad4f")])
def test_special_bits_are_the_ones_the_gpu_tests_always_drew(pool, seed, digest):
    v = B.special_bits(1000, seed, pool)
    assert v.dtype == np.float32 and v.shape == (1000,)
    assert hashlib.sha256(v.tobytes()).hexdigest()[:16] == digest


def test_diffuse_cases_draws_the_seed_99_array():
    from tests import diffuse_cases as DC
    assert DC.special_bits(1000).tobytes() == B.special_bits(1000, 99, B.POOL_TWELVE).tobytes()
    assert B.POOL_NINE.size == 9 and B.POOL_TWELVE.size == 12 and set(B.POOL_NINE) < set(B.POOL_TWELVE)


# ---- 4. the strictness of the comparers ---------------------------------------------------------------------------------------------
def records(dtype, n=6):
    rng = np.random.default_rng(5)
    p = np.zeros(n, dtype=dtype)
    for fld in FLOAT_FIELDS:
        p[fld] = rng.uniform(0.5, 2.0, size=p[fld].shape).astype(np.float32)
    p["grid"] = rng.integers(0, 1000, size=n)
    return p


def word(p, fld, k=3):
    """a writable u32 view of the first word of field `fld` of entry k"""
    return p[fld][k:k + 1].view(np.uint32).reshape(-1)[:1]


@pytest.mark.parametrize("dim", DTYPES)
def test_records_equal_to_themselves(dim):
    p = records(DTYPES[dim])
    B.assert_records_equal(p, p.copy(), "self")
    B.assert_records_equal(p, p.copy(), "self", nan_any=True)
    B.assert_records_equal(p[:0], p[:0].copy(), "empty")


@pytest.mark.parametrize("fld", FLOAT_FIELDS + ("grid",))
@pytest.mark.parametrize("dim", DTYPES)
def test_one_flipped_bit_in_one_field_raises(dim, fld):
    p = records(DTYPES[dim])
    q = p.copy()
    word(q, fld)[0] ^= 1                                # the lowest mantissa bit (of `grid`: the lowest bit)
    for nan_any in (False, True):
        with pytest.raises(AssertionError, match=f"ctx: {fld} not bit-exact in 1 of 6 entries; first 3"):
            B.assert_records_equal(q, p, "ctx", nan_any=nan_any)


@pytest.mark.parametrize("dim", DTYPES)
def test_zero_signs_nan_payloads_and_lengths(dim):
    p = records(DTYPES[dim])
    q = p.copy()
    p["density"][2], q["density"][2] = 0.0, -0.0
    with pytest.raises(AssertionError, match="density"):
        B.assert_records_equal(q, p, "signed zero")
    with pytest.raises(AssertionError, match="density"):
        B.assert_records_equal(q, p, "signed zero", nan_any=True)
    q = p.copy()
    word(p, "velocity")[0], word(q, "velocity")[0] = 0x7FC00000, 0xFFC12345
    with pytest.raises(AssertionError, match="velocity"):
        B.assert_records_equal(q, p, "payload")
    B.assert_records_equal(q, p, "payload", nan_any=True)            # two different NaNs
    word(q, "velocity")[0] = 0x3F800000
    with pytest.raises(AssertionError, match="velocity"):
        B.assert_records_equal(q, p, "a NaN against a number", nan_any=True)
    with pytest.raises(AssertionError, match="velocity"):
        B.assert_records_equal(p, q, "a number against a NaN", nan_any=True)
    for nan_any in (False, True):
        with pytest.raises(AssertionError, match="5 entries, expected 6"):
            B.assert_records_equal(p[:5], p, "length", nan_any=nan_any)


def test_pad_alone_is_not_compared():
    p = records(O.PARTICLE3_DTYPE)
    q = p.copy()
    q["pad"] = 0xDEADBEEF
    B.assert_records_equal(q, p, "pad")
    B.assert_records_equal(q, p, "pad", nan_any=True)


def test_same_words():
    a = np.array([1.0, np.nan, 0.0, np.nan, np.inf], dtype=np.float32)
    b = np.array([1.0, -np.nan, -0.0, 2.0, np.inf], dtype=np.float32)
    assert B.same_words(a, b).tolist() == [True, True, False, False, True]
    assert B.bits(np.float32([1.0, -0.0])).tolist() == [0x3F800000, 0x80000000]


def test_assert_identical():
    dt = np.dtype([("t", "<f4"), ("hit", "<u4")])
    a = np.zeros((3, 4), dtype=dt)
    B.assert_identical(a, a.copy(), "self")
    with pytest.raises(AssertionError, match="dtype"):
        B.assert_identical(a, a.astype(np.dtype([("t", "<f4"), ("steps", "<u4")])), "dtype")
    with pytest.raises(AssertionError, match="shape"):
        B.assert_identical(a, a.reshape(4, 3), "shape")
    with pytest.raises(AssertionError, match="shape"):
        B.assert_identical(a.ravel(), a, "shape")
    b = a.copy()
    b.view(np.uint8).reshape(-1)[8 * 7 + 3] = 1           # one byte of record 7
    with pytest.raises(AssertionError, match="1 of 12 records differ; first 7"):
        B.assert_identical(b, a, "byte")
    b = a.copy()
    b["t"][0, 0] = -0.0                                  # equal as a number, not in its bytes
    with pytest.raises(AssertionError, match="first 0"):
        B.assert_identical(b, a, "signed zero")


class Tracked:
    """what assert_track_equal reads of a handle (the methods) and of a checker (the attributes)"""

    def __init__(self, ids, attr):
        self.ids, self.attr, self.channels, self.track_channels = ids, attr, attr.shape[0], attr.shape[0]

    def particle_ids(self): return self.ids
    def attribute(self, c): return self.attr[c]


def test_assert_track_equal():
    ids = np.arange(8, dtype=np.uint32)[::-1].copy()
    attr = np.stack([B.special_bits(8, 1, B.POOL_TWELVE), np.arange(8, dtype=np.float32)])
    want = Tracked(ids, attr)
    B.assert_track_equal(Tracked(ids.copy(), attr.copy()), want, "self")            # NaNs included: bits, not values
    other = ids.copy()
    other[5] += 1
    with pytest.raises(AssertionError, match="ids differ in 1 slots"):
        B.assert_track_equal(Tracked(other, attr.copy()), want, "id")
    other = attr.copy()
    other[1].view(np.uint32)[4] ^= 1
    for nan_any in (False, True):
        with pytest.raises(AssertionError, match="channel 1 not bit-exact \\(1 words differ\\)"):
            B.assert_track_equal(Tracked(ids.copy(), other), want, "word", nan_any=nan_any)
    with pytest.raises(AssertionError, match="1 channels, expected 2"):
        B.assert_track_equal(Tracked(ids.copy(), attr[:1].copy()), want, "count")
    a, b = np.float32([[np.nan, 1.0]]), np.array([[0xFFC00001, 0x3F800000]], dtype=np.uint32).view(np.float32)
    two = np.arange(2, dtype=np.uint32)
    with pytest.raises(AssertionError, match="channel 0"):
        B.assert_track_equal(Tracked(two, a), Tracked(two, b), "payload")
    B.assert_track_equal(Tracked(two, a), Tracked(two, b), "payload", nan_any=True)
