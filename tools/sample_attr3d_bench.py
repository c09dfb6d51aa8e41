"""What the tracking channels cost in the 3D sampler: k3_sample_attr<C, GRID> for C = 1 and C = 4 beside k3_sample<GRID>
on the same queries, tools/sample3d_bench.py's three workloads after the 8 M dam_break_3d scene's window (10 warm-up + 100 steps):
the particles' own predicted positions in slot order (point form, a hipEvent pair on the simulation's stream: the kernel alone),
a 256^3 volume over the domain and a 2048^2 slice through the fluid (grid forms: blocking calls, so the event pair holds the
download too; the tiled kernels alone are read from a kernel trace of the same run, told apart by name and grid size).
Several alternated windows per variant, medians reported.

  python tools/sample_attr3d_bench.py [--n N] [--rounds R] [--reps K] [--volume V] [--slice S] [--out FILE]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/sample_attr3d_bench.py ...
  python tools/sample_attr3d_bench.py --summarise DIR/<name>_results.db | <name>_kernel_trace.csv [--out FILE]
                                                      (no GPU: medians per kernel and grid size, in microseconds)

No counters in the traced run.  Which unit bounds a kernel is not named here: only a separate --pmc run could name it.
"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=200 ** 3)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=3, help="launches per timed window of the point form")
ap.add_argument("--volume", type=int, default=256)
ap.add_argument("--slice", type=int, default=2048)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--summarise", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()


def emit(res):
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if a.summarise:
    groups = {}
    if a.summarise.endswith(".db"):                    # rocprofv3's default output: an SQLite file with a `kernels` view
        import sqlite3
        rows = sqlite3.connect(a.summarise).execute("select name, grid_x, start, end from kernels")
    else:                                              # --output-format csv
        rows = ((r["Kernel_Name"], r["Grid_Size_X"], r["Start_Timestamp"], r["End_Timestamp"]) for r in csv.DictReader(open(a.summarise)))
    for name, grid, start, end in rows:
        if "k3_sample" not in name and "k_track_carry" not in name and "k3_reorder" not in name:
            continue
        short = name.split("(")[0].replace("void ", "").replace("fsd::", "")
        groups.setdefault(f"{short} grid {grid}", []).append((int(end) - int(start)) / 1000.0)
    emit({k: {"launches": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
              "max_us": round(max(v), 2)} for k, v in sorted(groups.items())})
    sys.exit(0)

sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g

hip = C.CDLL("libamdhip64.so")


def ck(rc):
    if rc != 0:
        raise RuntimeError(f"HIP error {rc}")


def dev_alloc(nbytes):
    p = C.c_void_p()
    ck(hip.hipMalloc(C.byref(p), C.c_size_t(nbytes)))
    return p


settings, off, tick = g.dam_break_3d(a.n)
sim = g.FluidSimulation3D(settings, device=0, initial_offset=off)
sim.timed_steps(tick, a.warmup)
step_ms = sim.timed_steps(tick, a.steps) / a.steps
own = np.ascontiguousarray(sim.download_particles()["predicted_position"])
sx, sy, sz = float(settings.size.x), float(settings.size.y), float(settings.size.z)
zc = float(np.median(own[:, 2]))
views = {"volume": g._abi.View3(g.Vec3(-sx / 2, -sy / 2, -sz / 2), g.Vec3(sx / 2, sy / 2, sz / 2), a.volume, a.volume, a.volume),
         "slice": g._abi.View3(g.Vec3(-sx / 2, -sy / 2, zc), g.Vec3(sx / 2, sy / 2, zc), a.slice, a.slice, 1)}
voxels = {k: v.width * v.height * v.depth for k, v in views.items()}
d_own = dev_alloc(own.nbytes)
ck(hip.hipMemcpy(d_own, own.ctypes.data_as(C.c_void_p), C.c_size_t(own.nbytes), 1))
d_rec = dev_alloc(a.n * 40)
d_w = dev_alloc(a.n * 4)
d_a = dev_alloc(a.n * 16)
h_rec = np.zeros(max(voxels.values()), dtype=g.SAMPLE3_DTYPE)
h_w = np.zeros(max(voxels.values()), dtype=np.float32)
h_a = np.zeros(4 * max(voxels.values()), dtype=np.float32)
stream = C.c_void_p(sim.stream_ptr)
e0, e1 = C.c_void_p(), C.c_void_p()
ck(hip.hipEventCreate(C.byref(e0)))
ck(hip.hipEventCreate(C.byref(e1)))
P = lambda arr: arr.ctypes.data_as(C.c_void_p)      # noqa: E731
channels = {"c1": 1, "c4": 4}
current = [None]


def window(workload, variant):
    """ms per launch of one window.  variant: "sample" (k3_sample), "c1" / "c4" (k3_sample_attr with that many channels)."""
    if variant != "sample" and current[0] != variant:     # enable resets the channels: fill them again (values do not matter)
        sim.track(channels[variant])
        for c in range(channels[variant]):
            sim.set_attribute(c, own[:, c % 3])
        current[0] = variant
    reps = a.reps if workload == "own" else 1
    ck(hip.hipEventRecord(e0, stream))
    for _ in range(reps):
        if workload == "own":
            if variant == "sample":
                sim.sample_device(d_own.value, a.n, d_rec.value)
            else:
                sim.sample_attr_device(d_own.value, a.n, d_w.value, d_a.value)
        elif variant == "sample":
            g._check(sim._lib, sim._lib.fs3_sample_grid(sim._h, C.byref(views[workload]), P(h_rec)))
        else:
            g._check(sim._lib, sim._lib.fs3_sample_attr_grid(sim._h, C.byref(views[workload]), P(h_w), P(h_a)))
    ck(hip.hipEventRecord(e1, stream))
    ck(hip.hipEventSynchronize(e1))
    ms = C.c_float()
    ck(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
    return ms.value / reps


res = {"n": a.n, "warmup": a.warmup, "steps": a.steps, "step_ms": round(step_ms, 4), "reps": a.reps, "volume": a.volume,
       "slice": a.slice, "slice_z": zc, "grid_forms": "blocking calls: kernel + download (40 B per voxel for fs3_sample_grid, "
       "4 + 4 C for fs3_sample_attr_grid); the kernels alone: the kernel trace"}
variants = ["sample", "c1", "c4"]
for wl in ("own", "volume", "slice"):
    for v in variants:
        window(wl, v)                                  # first launch of each instantiation
        res[f"{wl}_{v}_ms"] = []
    for r in range(a.rounds):
        for v in variants[r % 3:] + variants[:r % 3]:
            res[f"{wl}_{v}_ms"].append(round(window(wl, v), 4))
    for v in variants:
        res[f"{wl}_{v}_median_ms"] = statistics.median(res[f"{wl}_{v}_ms"])
    res[f"{wl}_queries"] = a.n if wl == "own" else voxels[wl]
sim.sync()
sim.close()
emit(res)
