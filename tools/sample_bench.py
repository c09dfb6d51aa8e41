"""What field sampling costs: the 16 M dam break after bench.py's window (10 warm-up + 100 steps), then
fs_sample_points_device / fs_sample_grid's kernel timed with a hipEvent pair on the simulation's stream, several alternated
windows per query set, medians reported.  Query sets: M = N at the particles' own predicted positions in slot order with C = 0
and C = 4 channels, the same points shuffled, and a 2048 x 2048 grid over the domain (as points in row-major order: the
blocking fs_sample_grid adds a 100 MB download that is not the kernel's).

  python tools/sample_bench.py [--n N] [--rounds R] [--reps K] [--grid G] [--out FILE]

Run it under `rocprofv3 --kernel-trace --stats -- python tools/sample_bench.py ...` to read k_density and k_sample from one
trace.  Prints one JSON object (also written to --out).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1 << 24)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=3, help="launches per timed window")
ap.add_argument("--grid", type=int, default=2048)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--out", default=None)
a = ap.parse_args()

hip = C.CDLL("libamdhip64.so")


def ck(rc):
    if rc != 0:
        raise RuntimeError(f"HIP error {rc}")


def dev_alloc(nbytes):
    p = C.c_void_p()
    ck(hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)))
    return p


def upload(arr):
    arr = np.ascontiguousarray(arr)
    p = dev_alloc(arr.nbytes)
    ck(hip.hipMemcpy(p, arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes), 1))
    return p


settings, off, tick = g.dam_break_2d(a.n)
sim = g.FluidSimulation(settings, device=0, initial_offset=off, track=4)
rng = np.random.default_rng(1)
for c in range(4):
    sim.set_attribute(c, rng.uniform(-1.0, 1.0, a.n).astype(np.float32))
step_ms = sim.timed_steps(tick, a.warmup)
step_ms = sim.timed_steps(tick, a.steps) / a.steps
own = np.ascontiguousarray(sim.download_particles()["predicted_position"])
sx, sy = float(settings.size.x), float(settings.size.y)
f = np.float32
gi, gj = np.meshgrid(np.arange(a.grid, dtype=f), np.arange(a.grid, dtype=f))
gpts = np.stack([f(-sx / 2) + ((gi + f(0.5)) / f(a.grid)) * (f(sx / 2) - f(-sx / 2)),
                 f(-sy / 2) + ((gj + f(0.5)) / f(a.grid)) * (f(sy / 2) - f(-sy / 2))], axis=-1).reshape(-1, 2).astype(f)
sets = {"own_c0": (own, False), "own_c4": (own, True), "shuffled_c0": (own[rng.permutation(a.n)], False),
        "grid_c0": (gpts, False)}
dev = {k: upload(v[0]) for k, v in sets.items() if k != "own_c4"}
dev["own_c4"] = dev["own_c0"]
m_max = max(v[0].shape[0] for v in sets.values())
d_out, d_attr = dev_alloc(m_max * 24), dev_alloc(4 * m_max * 4)
stream = C.c_void_p(sim.stream_ptr)
e0, e1 = C.c_void_p(), C.c_void_p()
ck(hip.hipEventCreate(C.byref(e0)))
ck(hip.hipEventCreate(C.byref(e1)))


def window(name):
    pts, attr = sets[name]
    m = pts.shape[0]
    ck(hip.hipEventRecord(e0, stream))
    for _ in range(a.reps):
        sim.sample_device(dev[name].value, m, d_out.value, d_attr.value if attr else None)
    ck(hip.hipEventRecord(e1, stream))
    ck(hip.hipEventSynchronize(e1))
    ms = C.c_float()
    ck(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
    return ms.value / a.reps


res = {"n": a.n, "warmup": a.warmup, "steps": a.steps, "step_ms": round(step_ms, 4), "reps": a.reps, "grid": a.grid}
names = list(sets)
for name in names:
    window(name)                                   # first launch of each instantiation
    res[name + "_ms"] = []
for r in range(a.rounds):
    for name in names[r % len(names):] + names[:r % len(names)]:
        res[name + "_ms"].append(round(window(name), 4))
for name in names:
    res[name + "_median_ms"] = statistics.median(res[name + "_ms"])
    res[name + "_queries"] = int(sets[name][0].shape[0])
sim.sync()
sim.close()
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
