"""Fluid diagnostics without a GPU (include/fluidsim.h "fluid diagnostics"): the statement of tests/stats_ref.py on
hand-picked values, its freedom from order, crafted records whose words are written out by hand, the conditions of the cases the
GPU file runs (checked on the oracle), the layout of fs_stats / fs3_stats three ways, every layer of the bindings, and the CFL
helper of the Python record."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import layers
from tests import stats_cases as SC
from tests import stats_ref as R

f32 = np.float32
ROOT = layers.ROOT
CALLS_2D = ["fs_stats_read", "fs_stats_device"]
CALLS_3D = ["fs3_stats_read", "fs3_stats_device"]
METHODS = ["stats", "stats_device_ptr"]


def test_q_and_keys_on_hand_picked_values():
    ulp_below = np.nextafter(f32(16384.0), f32(0.0))
    ordered = f32([-np.inf, -np.finfo(f32).max, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, ulp_below, 16384.0, np.finfo(f32).max, np.inf])
    k = R.key(ordered).astype(np.int64)
    assert (np.diff(k) > 0).all(), "the key is not strictly monotone over the list"
    assert R.key(f32([-0.0]))[0] < R.key(f32([0.0]))[0] and R.key(f32([-0.0]))[0] == 0x7FFFFFFF and R.key(f32([0.0]))[0] == 0x80000000
    assert [R.unkey_bits(x) for x in R.key(ordered)] == [int(b) for b in R.bits(ordered)]
    assert R.unkey_bits(R.key(f32([np.inf]))[0]) == R.POS_INF and R.unkey_bits(R.key(f32([-np.inf]))[0]) == R.NEG_INF
    # Q: ties to even on both sides of zero, exact at the edge of the range
    assert R.B.Q(f32([R.TIE_LO, -R.TIE_LO, R.TIE_MID, -R.TIE_MID, R.TIE_HI, -R.TIE_HI])) == [0, 0, 2, -2, 2, -2]
    assert R.B.Q(f32([ulp_below])) == [(1 << 34) - (1 << 10)] and not R.B.in_range(f32([16384.0, np.nan, np.inf])).any()
    assert R.q_sum(f32([1.0, -0.5, 0.25])) == (1 << 20) - (1 << 19) + (1 << 18)
    big = np.random.default_rng(0).uniform(-16000, 16000, size=R.SMALL_Q + 5).astype(f32)
    assert R.q_sum(big) == sum(R.B.Q(big)), "the vectorised sum is not the sum of Q"


def test_reference_is_order_free(fs, orc):
    from tests import hard_states2d as H2
    case = H2.case_by_id(fs, orc, "nan_clamp")
    for rec in (case.start, case.run()[0].rec):
        attrs = list(SC.channel_values(rec.shape[0], 4))
        want = R.stats(rec, attrs, tick=3)
        perm = np.random.default_rng(1).permutation(rec.shape[0])
        R.assert_same(R.stats(rec[perm], [a[perm] for a in attrs], tick=3), want, "permuted")
        assert R.kept(want) >= 1


@pytest.mark.parametrize("dim", [2, 3])
def test_crafted_records_by_hand(fs, dim):
    dtype = fs.PARTICLE_DTYPE if dim == 2 else fs.PARTICLE3_DTYPE
    rec, attrs, want = R.crafted(dtype)
    R.assert_same(R.stats(rec, attrs), want, f"crafted {dim}D")
    assert rec["position"][1, 0] == 16384.0 and want["pos_max"][0] == R._fbits(16384.0) and want["dropped"] == 2
    assert want["speed2_max"] == R.POS_INF and want["nonfinite"] == 1
    rec, attrs, want = R.crafted_zeros(dtype)
    R.assert_same(R.stats(rec, attrs), want, f"zeros {dim}D")
    assert want["pos_min"] == (0x80000000,) * dim and want["pos_max"] == (0,) * dim


def test_scene_conditions(fs, orc):
    """what the GPU file's cases must show, on the oracle: a non-finite record, a dropped record and a dropped channel value
    somewhere, and in every state at least one record in the sums"""
    from tests import hard_states2d as H2
    from tests import hard_states3d as H3
    seen = {}
    for cid in SC.CASES_2D:
        case = H2.case_by_id(fs, orc, cid)
        states = [case.start] + [s.rec for s in case.run()[:SC.STEPS]]
        words = [R.stats(rec, list(SC.channel_values(case.n, 4))) for rec in states]
        assert all(R.kept(w) >= 1 for w in words), cid
        seen[cid] = words
    for cid in (SC.NONFINITE_3D, SC.DROPPED_3D):
        case = H3.case_by_id(fs, orc, cid)
        words = [R.stats(rec, list(SC.channel_values(case.n, 2))) for rec in [case.start] + list(case.run()[:SC.STEPS])]
        assert all(R.kept(w) >= 1 for w in words), cid
        seen[cid] = words
    after = lambda cid, k: max(w[k] for w in seen[cid][1:])
    assert after(SC.NONFINITE_2D, "nonfinite") > 0 and after(SC.NONFINITE_3D, "nonfinite") > 0
    assert after(SC.DROPPED_2D, "dropped") > 0 and after(SC.DROPPED_3D, "dropped") > 0
    assert seen["nan_clamp"][0]["nonfinite"] > 0 and seen["nan_clamp"][0]["dropped"] > 0       # the uploaded state itself
    assert all(w["attr_dropped"][1] > 0 for ws in seen.values() for w in ws)
    # the crafted sets: record counts by hand (test_crafted_records_by_hand); the empty-sums case is the one named so
    assert R.kept(R.crafted(fs.PARTICLE_DTYPE)[2]) == 2
    rec, _, want = R.crafted_empty(fs.PARTICLE_DTYPE)
    R.assert_same(R.stats(rec), want, "empty sums")
    assert R.kept(want) == 0 and want["speed2_max"] == R.NEG_INF and want["pos_min"] == (R.POS_INF, R.POS_INF)


def test_kernel_constants_match_the_test_file():
    text = open(os.path.join(layers.PKG, "csrc", "fs_kernels.h")).read()
    get = lambda name: int(re.search(rf"constexpr uint32_t {name} = (\d+)u;", text).group(1))
    assert (get("STATS_MAX_BLOCKS"), get("STATS_THREADS"), get("STATS_CHUNK")) == (SC.GRID_CAP, SC.THREADS, SC.CHUNK)


# ---- the layout, three ways -------------------------------------------------------------------------------------------------------
C_TYPES = {"uint64_t": (8, 8), "int64_t": (8, 8), "float": (4, 4), "uint32_t": (4, 4), "fs_vec2": (8, 4), "fs_vec3": (12, 4)}


def header_fields(struct):
    """[(name, offset, size)] of a struct of include/fluidsim.h, from the order of its fields and the C rules for the types above"""
    body = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (struct, struct), layers.header_text(), flags=re.S).group(1)
    out, off, align = [], 0, 1
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        size, al = C_TYPES[ctype]
        align = max(align, al)
        for name in (x.strip() for x in names.split(",")):
            m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", name)
            count = int(m.group(2) or 1)
            off = (off + al - 1) // al * al
            out.append((m.group(1), off, size * count))
            off += size * count
    return out, (off + align - 1) // align * align


@pytest.mark.parametrize("struct,ctype,size", [("fs_stats", "Stats", 208), ("fs3_stats", "Stats3", 232)])
def test_struct_layout(fs, struct, ctype, size, tmp_path):
    ct = getattr(fs._abi, ctype)
    fields, total = header_fields(struct)
    assert C.sizeof(ct) == size == total
    assert [f[0] for f in fields] == [f[0] for f in ct._fields_], "ctypes and the header name the fields in different orders"
    for name, off, sz in fields:
        assert (getattr(ct, name).offset, getattr(ct, name).size) == (off, sz), name
    # the same offsets in C99
    checks = "\n".join(f"    if (offsetof({struct}, {n}) != {o} || sizeof((({struct}*)0)->{n}) != {s}) return {i + 2};"
                       for i, (n, o, s) in enumerate(fields))
    src = tmp_path / "layout.c"
    src.write_text(f'#include <stddef.h>\n#include "fluidsim.h"\nint main(void) {{\n    if (sizeof({struct}) != {size}) return 1;\n'
                   f"{checks}\n    return FS_STATS_SHIFT == 20 ? 0 : 99;\n}}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    assert subprocess.run([str(exe)]).returncode == 0


def test_every_layer_names_the_calls(fs):
    layers.assert_every_layer_names(fs, CALLS_2D, fs.FluidSimulation, METHODS)
    layers.assert_every_layer_names(fs, CALLS_3D, fs.FluidSimulation3D, METHODS)
    for name in ("momentum", "kinetic_energy", "potential_energy", "centre_of_mass", "mean_density", "max_speed", "bounding_box",
                 "channel_sum", "channel_range", "healthy", "cfl_delta"):
        assert hasattr(fs.Stats, name) and hasattr(fs.Stats3D, name), name


# ---- the Python record ------------------------------------------------------------------------------------------------------------
def _raw(fs, **fields):
    raw = fs._abi.Stats()
    raw.speed2_max = -np.inf
    for k, v in fields.items():
        setattr(raw, k, v)
    return raw


def test_cfl_delta(fs):
    s = fs.Stats(_raw(fs, count=4, speed2_max=4.0))                 # largest speed 2
    assert s.max_speed() == 2.0
    assert s.cfl_delta(0.2) == pytest.approx(0.4 * 0.2 / 2.0, rel=1e-12)
    assert s.cfl_delta(0.5, courant=0.25) == pytest.approx(0.25 * 0.5 / 2.0, rel=1e-12)
    assert s.cfl_delta(0.2, floor=0.1) == 0.1 and s.cfl_delta(0.2, ceil=0.01) == 0.01
    assert s.cfl_delta(0.2, floor=0.001, ceil=1.0) == pytest.approx(0.04, rel=1e-12)
    for still in (fs.Stats(_raw(fs, count=4, speed2_max=0.0)), fs.Stats(_raw(fs, count=4, nonfinite=4))):   # at rest; nothing contributed
        assert still.max_speed() == 0.0 and still.cfl_delta(0.2, ceil=0.008) == 0.008
        with pytest.raises(ValueError):
            still.cfl_delta(0.2)
        with pytest.raises(ValueError):
            still.cfl_delta(0.2, floor=0.001)
    blown = fs.Stats(_raw(fs, count=1, dropped=1, speed2_max=np.inf))
    assert blown.cfl_delta(0.2) == 0.0 and blown.cfl_delta(0.2, floor=1e-4, ceil=1e-2) == 1e-4


def test_derived_quantities(fs):
    """the crafted record's words through the Python object: what the header says a host derives"""
    _, _, w = R.crafted(fs.PARTICLE_DTYPE)
    raw = _raw(fs, count=w["count"], nonfinite=w["nonfinite"], dropped=w["dropped"], energy_q=w["energy_q"], density_q=w["density_q"],
               speed2_max=np.inf, channels=2)
    raw.momentum_q[:] = w["momentum_q"]
    raw.position_q[:] = w["position_q"]
    raw.attr_q[:] = w["attr_q"]
    raw.attr_min[0], raw.attr_max[0] = -1.5 * 2.0 ** -20, 16384.0
    s = fs.Stats(raw)
    assert s.summed == 2 and not s.healthy
    assert s.momentum(2.0) == (2.0 * -3.0, 2.0 * (4.0 + 2 * 2.0 ** -20))
    assert s.kinetic_energy(2.0) == 25.0 and s.potential_energy(2.0, (0.0, 9.0)) == -2.0 * 9.0 * (-2.25 - 2 * 2.0 ** -20)
    assert s.centre_of_mass() == (0.75, (-2.25 - 2 * 2.0 ** -20) / 2) and s.mean_density() == (1000.5 + 2 * 2.0 ** -20) / 2
    assert s.channel_sum(0) == 3.0 - 2 * 2.0 ** -20 and s.channel_range(0) == (-1.5 * 2.0 ** -20, 16384.0)
    with pytest.raises(IndexError):
        s.channel_sum(2)
    assert fs.Stats.from_bytes(s.to_bytes()).momentum_q == s.momentum_q and len(s.to_bytes()) == 208
