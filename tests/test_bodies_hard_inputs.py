"""CPU companion of tests/test_bodies2d_hard_inputs_gpu.py and tests/test_bodies3d_hard_inputs_gpu.py: the cases of
tests/body_cases2d.py and tests/body_cases3d.py test what they say.  No GPU: the reference alone (the unchanged oracles plus the
numpy operators of tests/body_loads2d_ref.py and tests/body_loads3d_ref.py).  Every assertion is a condition on the cases; the
occurrence lists are printed with their case ids."""
import numpy as np
import pytest

from tests import body_cases2d as C2
from tests import body_cases3d as C3

f32 = np.float32


def _occurrences(runs, C, edges):
    """what the registry's runs hold, {name: [case ids]}; asserts the per-case and per-step conditions on the way.  `edges`: the
    slots of the edge bodies"""
    occ = {k: [] for k in ("cover re-clamps", "a later body re-clamps", "hit by two bodies", "edge particle reads the last pixel",
                           "last particle of an odd count hit", "NaN position left unchanged", "whirl drops, NaN velocity, a step after")}
    for cid, run in runs.items():
        n = run.case.n
        two = late = odd = nanpos = cover = whirl_ok = False
        edge_steps = 0
        for k, s in enumerate(run.steps):
            finite = C.finite_rows(s.before["position"])
            assert s.hits()[0] == int(finite.sum()), f"{cid} step {k + 1}: the cover body hits every finite particle"
            cover |= s.reclamped()[0] > 0
            late |= sum(s.reclamped()[1:]) > 0
            hit = np.stack([r["hit"] for r in s.recs])
            two |= bool((hit.sum(axis=0) >= 2).any())
            odd |= n % 2 == 1 and bool(hit[:, -1].any())
            nan = np.isnan(s.before["position"]).any(axis=1)
            if nan.any():
                assert not hit[:, nan].any(), f"{cid} step {k + 1}: a NaN position is outside every body"
                nanpos |= s.rec["position"][nan].tobytes() == s.before["position"][nan].tobytes()
            for e, slot in zip(s.edge, edges):
                if not C.finite_rows(s.edge_before[slot]["position"]).any():
                    continue
                assert e is not None, f"{cid} step {k + 1}: no edge particle for body {slot}"
                assert s.recs[slot]["hit"][e], f"{cid} step {k + 1}: the edge particle of body {slot} is not hit"
                assert C.on_edge_reads_last_pixel(s.bodies[slot], s.edge_before[slot]["position"][e]), f"{cid} step {k + 1} body {slot}"
                edge_steps += 1
            if "whirl" in run.names and k + 1 < len(run.steps):
                w = run.names.index("whirl")
                whirl_ok |= s.dropped()[w] > 0 and bool(np.isnan(s.rec["velocity"]).any())
        assert any(s.hits()[0] > 0 for s in run.steps)
        if "whirl" in run.names:
            assert whirl_ok, f"{cid}: the whirl must drop hits and leave a NaN velocity before the last step\n{C.describe(run)}"
            occ["whirl drops, NaN velocity, a step after"].append(cid)
        for name, flag in (("cover re-clamps", cover), ("a later body re-clamps", late), ("hit by two bodies", two),
                           ("edge particle reads the last pixel", edge_steps > 0), ("last particle of an odd count hit", odd),
                           ("NaN position left unchanged", nanpos)):
            if flag:
                occ[name].append(cid)
    return occ


def _print(tag, occ):
    for name, ids in occ.items():
        print(f"[{tag}] {name}: {len(ids)} cases: {ids}")


# ---- 2D ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs2(fs, orc):
    return {cid: C2.registry_run(fs, orc, cid) for cid in C2.CASE_IDS}


def test_registry2d_meets_its_conditions(runs2):
    occ = _occurrences(runs2, C2, [C2.NAMES.index("edge")])
    _print("body_cases2d", occ)
    for run in runs2.values():
        print(C2.describe(run))
    families = sorted({r.case.family for r in runs2.values() if r.case.n > 64})
    missing = [f for f in families if not any(c.split("/")[0] == f for c in occ["cover re-clamps"])]
    assert not missing, f"no re-clamp by the cover body in the families {missing}"
    assert set(occ["edge particle reads the last pixel"]) == set(C2.CASE_IDS)
    assert set(occ["hit by two bodies"]) == set(C2.CASE_IDS)
    assert occ["a later body re-clamps"] and occ["last particle of an odd count hit"] and occ["NaN position left unchanged"]
    assert occ["whirl drops, NaN velocity, a step after"] == C2.WHIRL_IDS
    small = {n: [cid for cid, r in runs2.items() if r.case.n == n] for n in (2, 3, 5)}
    print(f"[body_cases2d] the counts 2, 3 and 5: {small}")
    for n, ids in small.items():
        assert ids, f"no case of {n} particles"
        for cid in ids:
            assert all(sum(s.hits()) > 0 for s in runs2[cid].steps), f"{cid}: hits in every step"
    assert set(C2.AOS_IDS) <= set(C2.CASE_IDS) and set(C2.WHIRL_IDS) <= set(C2.AOS_IDS)


@pytest.fixture(scope="module")
def guard_base2(fs, orc):
    return C2.guard_base(fs, orc)


@pytest.mark.parametrize("name", C2.GUARD_IDS)
def test_guard2d_does_what_it_names(orc, guard_base2, name):
    """the guard's own check on the oracle's body-less step (the GPU file repeats it on the body-less handle's)"""
    st, off, tick, base = guard_base2
    g = C2.GUARDS[name]
    tk = g.tick(tick)
    ref = orc.OracleSim(st, off)
    ref.set_particles(g.upload(base))
    with np.errstate(all="ignore"):
        ref.step(tk)
        after = ref.particles()
        ref.close()
        bodies, want, words, recs = g.reference(after, (st.size.x, st.size.y), tk)
        print(f"[body_cases2d] guard {name}: {g.check(after, want, words, recs)}")
    assert base.shape[0] == 4097 and len(bodies) <= 8


def test_many_workgroups2d():
    for n, rows in zip(C2.MANY_WORKGROUPS, (2, 3)):
        groups = -(-n // C2.LOADS_WORKGROUP)
        assert n % 2 == 1 and -(-groups // C2.LOADS_SHARDS) == rows, "an odd count whose fullest shard row receives `rows` workgroups"


# ---- 3D ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs3(fs, orc):
    return {cid: C3.registry_run(fs, orc, cid) for cid in C3.CASE_IDS}


def test_registry3d_meets_its_conditions(runs3):
    occ = _occurrences(runs3, C3, [C3.NAMES.index("edge"), C3.NAMES.index("edge-z")])
    _print("body_cases3d", occ)
    for run in runs3.values():
        print(C3.describe(run))
    families = sorted({r.case.name.split("/")[0] for r in runs3.values() if r.case.n > 64})
    missing = [f for f in families if not any(c.split("/")[0] == f for c in occ["cover re-clamps"])]
    assert not missing, f"no re-clamp by the cover body in the families {missing}"
    assert set(occ["edge particle reads the last pixel"]) == set(C3.CASE_IDS)
    assert set(occ["hit by two bodies"]) == set(C3.CASE_IDS)
    assert occ["a later body re-clamps"] and occ["last particle of an odd count hit"] and occ["NaN position left unchanged"]
    assert occ["whirl drops, NaN velocity, a step after"] == C3.WHIRL_IDS


@pytest.fixture(scope="module")
def guard_base3(fs, orc):
    return C3.guard_base(fs, orc)


@pytest.mark.parametrize("name", C3.GUARD_IDS)
def test_guard3d_does_what_it_names(orc, guard_base3, name):
    st, off, tick, base = guard_base3
    g = C3.GUARDS[name]
    tk = g.tick(tick)
    ref = orc.OracleSim3D(st, off)
    ref.set_particles(g.upload(base))
    with np.errstate(all="ignore"):
        ref.step(tk)
        after = ref.particles()
        ref.close()
        bodies, want, words, recs = g.reference(after, (st.size.x, st.size.y, st.size.z), tk)
        print(f"[body_cases3d] guard {name}: {g.check(after, want, words, recs)}")
    assert base.shape[0] == 4097 and len(bodies) <= 8
