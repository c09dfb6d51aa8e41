"""CPU-side proof that the scenes of tests/csort_scenes.py reach the edges of the counting sort they are named after: for every
scene tests/test_csort_gpu.py parametrises over, the `facts` (cell keys from tests/pyref.py's xy_of_point on the f32 predicted
positions) say that the big cell has exactly the intended size, its slots sit where intended among the 256-slot workgroups, the
cell table has the intended length, the key runs occupy the intended lanes — and that the stable permutation is far from the
identity, so no GPU test can pass on an unsorted array.  No GPU."""
import numpy as np
import pytest

from tests import csort_scenes as S


def assert_not_vacuous(facts):
    if facts["cells"].size > 1:
        assert facts["moved"] > 0.5, "the stable permutation is (nearly) the identity: the scene shows nothing"


def assert_scattered(facts, big):
    """The members of a big cell come from all over the source array: every full 256-thread histogram workgroup holds some."""
    src = facts["perm"][big["lo"]:big["hi"]]
    assert np.all(np.diff(src.astype(np.int64)) > 0)                       # the stable order inside the cell
    assert np.unique(src // 256).size >= facts["n"] // 256


def assert_keeps_cells(st, tick, p, facts):
    """No particle changes cell in the predict step: the keys of the uploaded positions are the keys of the predicted ones."""
    still = p.copy()
    still["velocity"] = 0
    assert np.array_equal(S.cpu_keys(still, st, tick), facts["keys"])


@pytest.mark.parametrize("m,before,after", S.RANK_CASES)
def test_one_cell_has_exactly_m_particles(fs, m, before, after):
    st, tick, p, facts = S.one_cell(m, before, after)
    assert facts["n"] == st.particle_count == before + m + after == (12288 if m == 8193 else 8192)
    assert facts["counts"].max() == m and np.sort(facts["counts"])[-2] <= 4
    if m > S.RANK_MAX:
        (big,) = facts["big"]
        assert (big["m"], big["lo"], big["hi"]) == (m, before, before + m)
        assert_scattered(facts, big)
    else:
        assert facts["big"] == []
        k = facts["cells"][np.argmax(facts["counts"])]
        assert int((facts["keys"] < k).sum()) == before
    assert_keeps_cells(st, tick, p, facts)
    assert_not_vacuous(facts)


@pytest.mark.parametrize("m,before,after,lo_mod,ends", S.PLACEMENT_CASES)
def test_one_cell_sits_where_meant_among_the_workgroups(fs, m, before, after, lo_mod, ends):
    st, tick, p, facts = S.one_cell(m, before, after)
    (big,) = facts["big"]
    assert big["m"] == m and big["lo"] == before and big["lo_mod"] == lo_mod == before % 256
    assert (big["hi"] == facts["n"]) == ends
    if ends:
        assert after == 0 and facts["n"] % 256 == (lo_mod + m) % 256 and facts["n"] % 256 in (0, 1)
    assert_scattered(facts, big)
    assert_keeps_cells(st, tick, p, facts)
    assert_not_vacuous(facts)


def test_placements_cover_every_residue_and_both_array_ends():
    assert {c[3] for c in S.PLACEMENT_CASES if not c[4]} == {0, 1, 255}
    assert {(c[1] + c[0]) % 256 for c in S.PLACEMENT_CASES if c[4]} == {0, 1}


@pytest.mark.parametrize("m_a,m_b,before,lo_b_mod", S.TWO_CASES)
def test_two_cells_are_back_to_back_in_one_workgroup(fs, m_a, m_b, before, lo_b_mod):
    st, tick, p, facts = S.two_cells(m_a, m_b, before)
    top = np.argsort(facts["counts"])[-2:]
    a, b = sorted(top)
    assert b == a + 1, "an occupied cell lies between the two"
    assert (facts["counts"][a], facts["counts"][b]) == (m_a, m_b) and np.sort(facts["counts"])[-3] <= 4
    lo_a = int(facts["counts"][:a].sum())
    hi_a = lo_a + m_a
    lo_b = hi_a                                                            # consecutive occupied keys
    assert lo_a == before and lo_b % 256 == lo_b_mod != 0
    assert lo_b // 256 == (hi_a - 1) // 256                                # one workgroup: A's tail and B's first slot
    assert [c["m"] for c in facts["big"]] == [m for m in (m_a, m_b) if m > S.RANK_MAX]
    for big in facts["big"]:
        assert_scattered(facts, big)
    # no geometric neighbours: at least 3 rows apart
    gw = facts["grid"][0]
    assert int(facts["cells"][b]) // gw - int(facts["cells"][a]) // gw >= 3
    assert_keeps_cells(st, tick, p, facts)
    assert_not_vacuous(facts)


@pytest.mark.parametrize("n", S.ALL_CASES)
def test_all_in_one_is_one_cell(fs, n):
    st, tick, p, facts = S.all_in_one(n)
    assert facts["cells"].size == 1 and facts["big"] == [{"key": int(facts["cells"][0]), "m": n, "lo": 0, "hi": n, "lo_mod": 0}]
    assert -(-n // 256) >= 9                                               # every workgroup but the first only waits
    assert_keeps_cells(st, tick, p, facts)


@pytest.mark.parametrize("n", S.LATTICE_N)
def test_lattice_scenes_are_ragged_and_shuffled(fs, n):
    st, tick, p, facts = S.lattice(n)
    assert facts["n"] == n == st.particle_count
    assert facts["big"] == []
    assert_not_vacuous(facts)
    if n > 3:
        assert facts["cells"].size > 1


def test_lattice_sizes_sit_on_both_sides_of_every_block_size():
    for block in (64, 256, 1024):
        assert {block - 1, block, block + 1} <= set(S.LATTICE_N)
    assert {n % 1024 for n in S.LATTICE_N} >= {1023, 0, 1} and min(S.LATTICE_N) == 2


@pytest.mark.parametrize("gw,gh,count,tiles", S.TABLE_CASES)
def test_table_has_the_intended_length_and_corners(fs, gw, gh, count, tiles):
    st, tick, p, facts = S.table(gw, gh)
    assert facts["grid"] == S.formula_grid(st) == (gw, gh)
    assert facts["scan_count"] == gw * gh + 1 == count and facts["scan_tiles"] == tiles == -(-count // 16384)
    assert facts["n"] == 3000 and facts["counts"].max() <= 4
    assert facts["keys"][facts["corner_lo"]] == gw + 1 == facts["keys"].min()           # cx = cy = 1
    assert facts["keys"][facts["corner_hi"]] == gw * gh - 1 == facts["keys"].max()      # the table's last key
    # (a last tile of ONE item holds the grand total's slot alone and no cell: then the last cell's tile is the one before it)
    assert facts["tile_occupied"][0] and facts["tile_occupied"][(gw * gh - 1) // 16384]
    assert (gw * gh - 1) // 16384 == tiles - (2 if count % 16384 == 1 else 1)
    if tiles > 65:
        assert facts["longest_empty_tiles"] >= 64
    assert_not_vacuous(facts)


def test_tables_cover_the_thread_and_tile_edges():
    counts = [c[2] for c in S.TABLE_CASES]
    assert {c % 16 for c in counts} >= {0, 1, 15}
    assert {16384, 16385, 32768, 32769} <= set(counts)
    assert any(c % 16384 == 1 for c in counts)                             # a last tile of one item
    assert any(c[3] > 65 for c in S.TABLE_CASES) and any(c[3] > 129 for c in S.TABLE_CASES)


def _runs_of(facts, wave):
    return [(a, l, k) for w, a, l, k in facts["lane_runs"] if w == wave]


@pytest.mark.parametrize("pattern", S.RUN_PATTERNS)
def test_runs_occupy_the_intended_lanes(fs, pattern):
    st, tick, p, facts = S.runs(pattern)
    n, runs = facts["n"], facts["lane_runs"]
    assert facts["counts"].max() <= 200
    # every label has a cell of its own: the key runs are the label runs
    assert [r[:3] for r in S.lane_runs(facts["labels"])] == [r[:3] for r in runs]
    assert np.unique(facts["keys"]).size == np.unique(facts["labels"]).size
    if pattern == "full_wave":
        assert [len(_runs_of(facts, w)) for w in range(4)] == [1, 1, 1, 1]
        assert _runs_of(facts, 0)[0][2] == _runs_of(facts, 2)[0][2] != _runs_of(facts, 1)[0][2]
    elif pattern == "ends_at_63":
        a, l, k = _runs_of(facts, 0)[-1]
        assert a + l == 64 and l < 64 and _runs_of(facts, 1)[0][2] != k and _runs_of(facts, 1)[0][1] < 64
    elif pattern == "continues":
        for w in (0, 1, 2):
            assert _runs_of(facts, w)[-1][2] == _runs_of(facts, w + 1)[0][2]
        assert _runs_of(facts, 2) == [(0, 64, _runs_of(facts, 1)[-1][2])]
    elif pattern == "alternating":
        assert [l for _, l, _ in _runs_of(facts, 0) + _runs_of(facts, 1) + _runs_of(facts, 2)] == [1] * 192
        assert len({k for _, _, k in _runs_of(facts, 0)}) == 2
    elif pattern == "lengths_1_to_64":
        lab = facts["labels"]
        cut = np.concatenate([[0], np.nonzero(lab[1:] != lab[:-1])[0] + 1, [n]])
        assert np.array_equal(np.diff(cut), np.arange(1, 65))
        assert any(a + l == 64 for _, a, l, _ in runs) and n == 2080
    elif pattern == "ragged_1":
        assert n % 64 == 1 and _runs_of(facts, n // 64) == [(0, 1, _runs_of(facts, n // 64 - 1)[-1][2])]
    elif pattern == "ragged_63":
        a, l, k = _runs_of(facts, n // 64)[-1]
        assert n % 64 == 63 and a + l == 63
    assert_not_vacuous(facts)


def test_slab_scene_puts_one_big_cell_inside_rank_0_and_one_at_the_boundary(fs, orc):
    st, tick, p, facts = S.slab_two_big_cells()
    assert facts["n"] == 16384 and [b["m"] for b in facts["big"]] == [2500, 2500]
    assert np.sort(facts["counts"])[-3] <= 4
    lo, mid, hi = facts["bounds"]
    assert (lo, hi) == (0, facts["grid"][0])
    assert facts["col_a"] < mid - 8                                        # interior of rank 0, far from the halo and edge zones
    assert mid - 2 <= facts["col_b"] < mid                                 # owned by rank 0 and sent to rank 1 as halo
    gw = facts["grid"][0]
    assert sorted(b["key"] % gw for b in facts["big"]) == [facts["col_a"], facts["col_b"]]
    assert_keeps_cells(st, tick, p, facts)
    assert_not_vacuous(facts)
    # the tick's force terms vanish exactly: one oracle step is v += g dt, bit for bit (density is the only float left that
    # depends on the order of summation)
    ref = orc.OracleSim(st, ref_quirks=False)
    ref.set_particles(p)
    ref.step(tick, stable_sort=True)
    got = ref.particles()
    g_dt = (np.float32([tick.gravity.x, tick.gravity.y]) * np.float32(tick.delta)).astype(np.float32)
    want = (p["velocity"][facts["perm"]] + g_dt).astype(np.float32)
    assert np.array_equal(got["velocity"].view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got["grid"], facts["keys"][facts["perm"]])
    ref.close()
