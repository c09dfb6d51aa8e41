"""The loops of the 2D force walk, its scan and the density row loop on their exits (csrc/fs_force_sweep.h, kernels_force_quad.inc,
kernels_density.hip DensityTerms::row) and the shared-reciprocal terms without a `dst <= h` test of their own (fs_force_pair.h): the
scenes of tests/walk_diet_scenes.py — whose edges tests/test_walk_diet_scenes.py proves on the CPU — in strict mode, three steps,
every field of every particle and start_indices bit for bit against the oracle.

Each scene runs through the default kernel choice, with k_force_quad in every step (FS_FORCE_QUAD_ALWAYS=1), and on a handle whose
force pass keeps its true divisions (FS_NO_SHAREDIV=1 is read once per process: one child runs every scene)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import walk_diet_scenes as W
from tests.bitcmp import assert_records_equal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_against_oracle(fs, name, ctx):
    st, ticks, p = W.scene(name)
    states, _ = W.oracle_states(name)
    sim = fs.FluidSimulation(st, device=0)
    sim.upload_particles(p)
    for s, tick in enumerate(ticks):
        sim.tick(tick)
        want, start = states[s]
        assert_records_equal(sim.download_particles(), want, f"{ctx} {name} step {s}")
        assert np.array_equal(sim.download_start_indices(), start), f"{ctx} {name} step {s}: start_indices"
    sim.close()


@pytest.mark.parametrize("name", W.NAMES)
def test_default_kernel_choice(fs, orc, name):
    run_against_oracle(fs, name, "default")


@pytest.mark.parametrize("name", W.NAMES)
def test_quad_kernel_in_every_step(fs, orc, monkeypatch, name):
    monkeypatch.setenv("FS_FORCE_QUAD_ALWAYS", "1")         # read when the handle is created
    run_against_oracle(fs, name, "quad")


CHILD = r'''
import os, sys
sys.path.insert(0, os.getcwd())
import numpy as np
import gpu_fluid_simulation_amd as fs
from tests import walk_diet_scenes as W
from tests.bitcmp import assert_records_equal
for name in W.NAMES:
    st, ticks, p = W.scene(name)
    states, _ = W.oracle_states(name)
    sim = fs.FluidSimulation(st, device=0)
    assert fs.load_library().fs_constdiv_status(sim._h) & 12 == 0, "shared path should be off"
    sim.upload_particles(p)
    try:
        for s, tick in enumerate(ticks):
            sim.tick(tick)
            assert_records_equal(sim.download_particles(), states[s][0], f"step {s}")
            assert np.array_equal(sim.download_start_indices(), states[s][1]), f"step {s}: start_indices"
        print("ok", name, flush=True)
    except AssertionError as e:
        print("FAILED", name, e, flush=True)
    sim.close()
'''


@pytest.fixture(scope="module")
def true_division_child(fs, orc):
    env = dict(os.environ, FS_NO_SHAREDIV="1")
    out = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.splitlines()


@pytest.mark.parametrize("name", W.NAMES)
def test_true_division_path(true_division_child, name):
    assert f"ok {name}" in true_division_child, [l for l in true_division_child if name in l]
