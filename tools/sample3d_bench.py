"""What 3D field sampling costs: the 8 M dam_break_3d scene after its window (10 warm-up + 100 steps), then
the sampler timed with a hipEvent pair on the simulation's stream, several alternated windows per query set, medians reported.
Query sets: M = N at the particles' own predicted positions in slot order, the same points shuffled, a 256^3 volume over the
domain and a 2048^2 slice through the fluid.  The two grids are timed twice: their voxel centres as points in row-major order
through fs3_sample_points_device (event pair: the kernel alone), and fs3_sample_grid itself (event pair around the blocking
call: the tiled kernel PLUS its download of 40 bytes per voxel; the tiled kernel alone is k3_sample<true> in a kernel trace,
the two views told apart by their grid sizes).

  python tools/sample3d_bench.py [--n N] [--rounds R] [--reps K] [--volume V] [--slice S] [--out FILE]

Run it under `rocprofv3 --kernel-trace --stats -- python tools/sample3d_bench.py ...` to read k3_density and k3_sample from one
trace (no counters in that run).  Prints one JSON object (also written to --out).  Which unit bounds the kernel is not named
here: only a separate --pmc run could name it.
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
ap.add_argument("--n", type=int, default=200 ** 3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=3, help="launches per timed window")
ap.add_argument("--volume", type=int, default=256)
ap.add_argument("--slice", type=int, default=2048)
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


def voxel_centres(width, height, depth, wmin, wmax):
    f = np.float32
    axes = [f(lo) + ((np.arange(cnt, dtype=f) + f(0.5)) / f(cnt)) * (f(hi) - f(lo)) for cnt, lo, hi in
            zip((width, height, depth), wmin, wmax)]
    k, j, i = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([i, j, k], axis=-1).reshape(-1, 3).astype(f)


settings, off, tick = g.dam_break_3d(a.n)
sim = g.FluidSimulation3D(settings, device=0, initial_offset=off)
sim.timed_steps(tick, a.warmup)
step_ms = sim.timed_steps(tick, a.steps) / a.steps
own = np.ascontiguousarray(sim.download_particles()["predicted_position"])
sx, sy, sz = float(settings.size.x), float(settings.size.y), float(settings.size.z)
zc = float(np.median(own[:, 2]))
views = {"volume": (a.volume, a.volume, a.volume, (-sx / 2, -sy / 2, -sz / 2), (sx / 2, sy / 2, sz / 2)),
         "slice": (a.slice, a.slice, 1, (-sx / 2, -sy / 2, zc), (sx / 2, sy / 2, zc))}
rng = np.random.default_rng(1)
sets = {"own": own, "shuffled": own[rng.permutation(a.n)]}
for name, v in views.items():
    sets[name + "_as_points"] = voxel_centres(*v)
dev = {k: upload(v) for k, v in sets.items()}
m_max = max(v.shape[0] for v in sets.values())
d_out = dev_alloc(m_max * 40)
host = {name: np.zeros(v[0] * v[1] * v[2], dtype=g.SAMPLE3_DTYPE) for name, v in views.items()}
stream = C.c_void_p(sim.stream_ptr)
e0, e1 = C.c_void_p(), C.c_void_p()
ck(hip.hipEventCreate(C.byref(e0)))
ck(hip.hipEventCreate(C.byref(e1)))


def window(name):
    ck(hip.hipEventRecord(e0, stream))
    if name in views:                                  # the blocking grid form: kernel + download
        w, h, d, wmin, wmax = views[name]
        view = g._abi.View3(g.Vec3(*wmin), g.Vec3(*wmax), w, h, d)
        for _ in range(a.reps):
            g._check(sim._lib, sim._lib.fs3_sample_grid(sim._h, C.byref(view), host[name].ctypes.data_as(C.c_void_p)))
    else:
        for _ in range(a.reps):
            sim.sample_device(dev[name].value, sets[name].shape[0], d_out.value)
    ck(hip.hipEventRecord(e1, stream))
    ck(hip.hipEventSynchronize(e1))
    ms = C.c_float()
    ck(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
    return ms.value / a.reps


res = {"n": a.n, "warmup": a.warmup, "steps": a.steps, "step_ms": round(step_ms, 4), "reps": a.reps, "volume": a.volume,
       "slice": a.slice, "slice_z": zc}
names = list(sets) + [name for name in views]
for name in names:
    window(name)                                   # first launch of each instantiation
    res[name + "_ms"] = []
for r in range(a.rounds):
    for name in names[r % len(names):] + names[:r % len(names)]:
        res[name + "_ms"].append(round(window(name), 4))
for name in names:
    res[name + "_median_ms"] = statistics.median(res[name + "_ms"])
    res[name + "_queries"] = int(host[name].shape[0] if name in views else sets[name].shape[0])
for name in views:
    res[name + "_hit_fraction"] = round(float((host[name]["neighbours"] > 0).mean()), 4)
sim.sync()
sim.close()
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
