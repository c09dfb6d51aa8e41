"""bench.py's single-GPU line: a plain run prints only the headline, `--full` adds the roofline and the other
measurements, and `--dump-outputs DIR` writes what the timed path computed in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402  (tests/conftest.py puts the repository root on sys.path)

EXTRAS = ("roofline", "cpu_baseline", "alt_modes", "alt_windows", "alt_workloads")


class _FakeSim:
    def __init__(self, particles, starts=None):
        self._p, self._s = particles, starts
        if starts is not None:
            self.download_start_indices = lambda: self._s

    def download_particles(self):
        return self._p


def _records(dtype, n, seed):
    rng = np.random.default_rng(seed)
    a = np.zeros(n, dtype=dtype)
    for f in dtype.names:
        a[f] = rng.random(a[f].shape) if a[f].dtype.kind == "f" else rng.integers(0, 2**32, a[f].shape, dtype=np.uint64)
    return a


def test_dump_outputs_fields_types_and_seeded_sample(tmp_path, monkeypatch):
    import gpu_fluid_simulation_amd as g
    monkeypatch.setattr(bench, "DUMP_ROWS", 64)
    parts = _records(g.PARTICLE_DTYPE, 1000, 1)
    starts = np.random.default_rng(2).integers(0, 2**32, 40, dtype=np.uint64).astype(np.uint32)
    bench.dump_outputs(_FakeSim(parts, starts), str(tmp_path / "a"))
    bench.dump_outputs(_FakeSim(parts, starts), str(tmp_path / "b"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted([f"particles_{f}.npy" for f in g.PARTICLE_DTYPE.names] + ["start_indices.npy"])
    pos = np.load(tmp_path / "a" / "particles_position.npy")
    assert pos.dtype == np.float32 and pos.shape == (64, 2)
    rows = np.flatnonzero(np.isin(parts["position"][:, 0], pos[:, 0]))
    assert rows.shape[0] == 64 and np.array_equal(parts["position"][rows], pos)      # a sample of rows, in row order
    grid = np.load(tmp_path / "a" / "particles_grid.npy")
    assert grid.dtype == np.float64 and np.array_equal(grid, parts["grid"][rows].astype(np.float64))   # u32 kept exactly
    si = np.load(tmp_path / "a" / "start_indices.npy")
    assert si.dtype == np.float64 and np.array_equal(si, starts.astype(np.float64))   # short enough: all of it
    for n in names:                                                                   # the same sample every run
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))


def test_dump_outputs_3d_drops_padding_and_stays_under_64_mb(tmp_path, monkeypatch):
    import gpu_fluid_simulation_amd as g
    monkeypatch.setattr(bench, "DUMP_ROWS", 16)
    bench.dump_outputs(_FakeSim(_records(g.PARTICLE3_DTYPE, 100, 3)), str(tmp_path))
    names = sorted(os.listdir(tmp_path))
    assert names == sorted(f"particles_{f}.npy" for f in g.PARTICLE3_DTYPE.names if f != "pad")
    bytes_per_row = sum(np.load(tmp_path / n).nbytes for n in names) // 16
    monkeypatch.undo()
    assert bytes_per_row * bench.DUMP_ROWS <= 64e6          # the widest record, at the real sample size


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_fresh_library_is_loaded_without_the_build_lock(fs, monkeypatch):
    """A built checkout may be read-only to the user who runs the benchmark: with the library up to date, bench.py
    loads it without build_product(), which opens the build lock for writing."""
    import __graft_entry__ as ge
    assert not ge.product_is_stale()
    monkeypatch.setattr(ge, "build_product", lambda: pytest.fail("build_product() called for an up-to-date library"))
    assert bench.load_product(False).load_library() is fs.load_library()


def _bench(*argv, timeout=600):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--no-build", "--workload", "dam_break_2d_4096"] + list(argv),
                       capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(fs, tmp_path):
    """A plain run: the headline fields and nothing else; its dump equals a fresh handle stepped warm-up + steps times,
    and is the same in a second run."""
    outs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        out = _bench("--steps", "3", "--warmup", "2", "--dump-outputs", str(d))
        assert out["steps"] == 3 and out["warmup"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0
        assert out["metric"] == out["unit"] == "M particle-steps/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
        assert not any(x in out for x in EXTRAS)
        outs.append({n[:-4]: np.load(d / n) for n in os.listdir(d)})
    st, off, tick = fs.dam_break_2d(4096)
    sim = fs.FluidSimulation(st, device=0, initial_offset=off)
    for _ in range(5):
        sim.tick(tick)
    sim.sync()
    want, starts = sim.download_particles(), sim.download_start_indices()
    sim.close()
    assert sorted(outs[0]) == sorted([f"particles_{f}" for f in want.dtype.names] + ["start_indices"])
    for f in want.dtype.names:
        assert np.array_equal(outs[0][f"particles_{f}"], want[f].astype(outs[0][f"particles_{f}"].dtype)), f
    assert np.array_equal(outs[0]["start_indices"], starts.astype(np.float64))
    for name, a in outs[0].items():
        assert np.array_equal(a, outs[1][name]), name


@pytest.mark.gpu
def test_full_bench_line_has_the_roofline(fs):
    """--full re-runs the headline window with per-pass events; a window longer than FULL_STEPS is re-run only up to
    there, so that a long headline window does not multiply the cost of --full."""
    out = _bench("--steps", "3", "--warmup", "2", "--full", "--no-alt", "--no-cpu-baseline")
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    assert set(out["roofline"]["passes"]) == {"sort", "reorder", "density", "force"}
    assert out["roofline"]["profiled_ms_per_step"] > 0 and out["roofline"]["profiled_window"] == "steps 2..5 from the lattice"
    out = _bench("--steps", str(bench.FULL_STEPS + 50), "--warmup", "2", "--full", "--no-alt", "--no-cpu-baseline")
    assert out["steps"] == bench.FULL_STEPS + 50
    assert out["roofline"]["profiled_window"] == f"steps 2..{2 + bench.FULL_STEPS} from the lattice"
