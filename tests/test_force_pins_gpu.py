"""The force pass's two non-strict math modes, pinned bit for bit.

FS_MATH_WGSL_ULP and FS_MATH_TOLERANCE are otherwise held to a tolerance only (test_parity_gpu.py,
test_surface_tension_gpu.py): a change of the force kernels that moved their bits would pass there.  Here four steps of the
dense scene (tests/dense_scene.py: every sweep path, both deferred-wave lists, coincident pairs) are pinned by the SHA-256
of the downloaded particle records and of start_indices after each step.  The strict mode is pinned by the oracle instead,
and in every mode a handle with a registered export (the AOS instantiations of the force kernels) must produce the plain
handle's bytes.

PINS was recorded on an MI355X from the library of commit 46c36b7 ("3D step: opt-in particle tracking, and its channels in
the 3D sampler"), the parent of the split of kernels_force.hip, twice in two processes with equal results.  A deliberate
change of either mode's arithmetic re-records them; nothing else may."""
import hashlib

import numpy as np
import pytest

from tests.dense_scene import dense_scene

pytestmark = pytest.mark.gpu
STEPS = 4

# per step: (sha256 of download_particles().tobytes(), sha256 of download_start_indices().tobytes())
PINS = {
    "ulp": [
        ("21efe05097d6ab57e8d83e56fc90f8a7439ccb08e1262471bf19882a90ea7c20",
         "b37ff68cc4d36f42a609839742b520687311368087bd842377095ffbbb0a6d9f"),
        ("bd5dcf06fc98564e31aa3ff3ef1ca374f648f63d46c8c9cffcfff21f6fe61a2b",
         "4ec99472629ae22cd7715c4d49a1e76b1f23e9357006c9dba13e6feeb84c1786"),
        ("ed0a20c8b9d6af792d63c2b9d60912be2a74286627d59bf91ef364a9d12f55e5",
         "3a6a80c2445e0f2225e6a82076790f109c42edfb251832eccef8ed3780a15cca"),
        ("d715fef5c4d8e93aa91445a49d894c3553b38db49ab9d22ca79243e2485cb32f",
         "fd1054a300db49717f97aef23d7636bc240ddda35b9ef4451525c912d932555b"),
    ],
    "tolerance": [
        ("e0bdba2948c22c2937035f2b46e6d0d1c07e3512c287dda7b7ed35a65a56d7c6",
         "b37ff68cc4d36f42a609839742b520687311368087bd842377095ffbbb0a6d9f"),
        ("9cc414b4124e66fb17688e707f2f31e745dd11e3bbab4ca5a70e83725a9ec307",
         "4ec99472629ae22cd7715c4d49a1e76b1f23e9357006c9dba13e6feeb84c1786"),
        ("1698391cfa4cb24b0f1d980160163b315b4bde6d56af5a9f90359e6677b447e4",
         "3a6a80c2445e0f2225e6a82076790f109c42edfb251832eccef8ed3780a15cca"),
        ("677f5c6f4ea059373d13dc8b866ccdfeb4eda8b16560968b368527655bb3e2a8",
         "fd1054a300db49717f97aef23d7636bc240ddda35b9ef4451525c912d932555b"),
    ],
}
PINS["ulp-quad"] = PINS["ulp"]      # as recorded: the quad kernel changes no bit (test_parity_gpu.py pins that too)


def math_mode(fs, math):
    return {"ieee": fs.FS_MATH_IEEE, "ulp": fs.FS_MATH_WGSL_ULP, "tolerance": fs.FS_MATH_TOLERANCE}[math]


def run_case(fs, math, aos=False):
    """The state after each of STEPS steps of the dense scene: [(particle records, start_indices)].  `aos`: an export
    handle is taken before the first step, so the force pass writes the records itself."""
    st, tick, p = dense_scene(fs)
    sim = fs.FluidSimulation(st, device=0, math_mode=math_mode(fs, math))
    sim.upload_particles(p)
    if aos:
        sim.export_handle()
    out = []
    for _ in range(STEPS):
        sim.tick(tick)
        out.append((sim.download_particles(), sim.download_start_indices()))
    sim.close()
    return out


def digests(states):
    return [(hashlib.sha256(a.tobytes()).hexdigest(), hashlib.sha256(b.tobytes()).hexdigest()) for a, b in states]


@pytest.fixture(scope="module")
def plain(fs):
    """The plain handle's states per math mode, computed once and never written to."""
    cache = {}

    def get(math):
        if math not in cache:
            cache[math] = run_case(fs, math)
        return cache[math]
    return get


@pytest.mark.parametrize("math", ["ulp", "tolerance"])
def test_default_knobs_pinned(plain, math):
    got = digests(plain(math))
    assert got == PINS[math]


def test_quad_kernel_pinned(fs, monkeypatch):
    """FS_FORCE_QUAD_ALWAYS=1: k_force_quad takes the pre-registered list in every step."""
    monkeypatch.setenv("FS_FORCE_QUAD_ALWAYS", "1")
    got = digests(run_case(fs, "ulp"))
    assert got == PINS["ulp-quad"]


@pytest.mark.parametrize("math", ["ieee", "ulp", "tolerance"])
def test_aos_instantiations_change_no_byte(fs, plain, math):
    got, want = run_case(fs, math, aos=True), plain(math)
    for s in range(STEPS):
        assert got[s][0].tobytes() == want[s][0].tobytes(), f"{math} step {s}: particle records"
        assert got[s][1].tobytes() == want[s][1].tobytes(), f"{math} step {s}: start_indices"


def test_strict_mode_against_oracle(fs, orc, plain):
    from tests.test_parity_gpu import assert_particles_equal
    st, tick, p = dense_scene(fs)
    ref = orc.OracleSim(st)
    ref.set_particles(p)
    for s, (particles, start) in enumerate(plain("ieee")):
        ref.step(tick)
        assert_particles_equal(particles, ref.particles(), f"dense/ieee step {s}")
        assert np.array_equal(start, ref.start_indices()), f"dense/ieee step {s}: start_indices"
    ref.close()
