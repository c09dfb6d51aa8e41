"""What the opt-in 3D particle tracking costs: the 8 M dam_break_3d over bench.py's window (10 warm-up + 100 timed
steps, from a fresh handle) with tracking off, with ids only (C = 0) and with four channels (C = 4), alternated, each round
starting with another setting; then one window per setting with pass events (the carry falls inside the reorder interval).

  python tools/ab_track3d.py [--n N] [--rounds R] [--warmup W] [--steps K] [--parent-lib FILE] [--out FILE]

--parent-lib: a library built from the parent commit (it lacks the fs3_track_* symbols, so it is driven through bare ctypes):
its windows are alternated with the others as setting "parent", to tell whether tracking OFF costs anything.
Prints one JSON object (also written to --out): ms per step of every window, the medians, the per-pass times.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=200 ** 3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()

SETTINGS = [("off", None), ("c0", 0), ("c4", 4)]
parent = None
if a.parent_lib:
    parent = C.CDLL(os.path.abspath(a.parent_lib))
    parent.fs3_create_ex.argtypes = [C.c_void_p, C.c_int, g.Vec3, C.c_int, C.c_void_p]
    parent.fs3_timed_steps.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    parent.fs3_destroy.argtypes = [C.c_void_p]
    parent.fs3_destroy.restype = None
    SETTINGS.insert(0, ("parent", None))


def parent_window():
    settings, off, tick = g.dam_break_3d(a.n)
    h, ms = C.c_void_p(), C.c_double()
    assert parent.fs3_create_ex(C.byref(settings), 0, g.Vec3(*off), g.FS_MATH_IEEE, C.byref(h)) == 0
    assert parent.fs3_timed_steps(h, C.byref(tick), a.warmup, C.byref(ms)) == 0
    assert parent.fs3_timed_steps(h, C.byref(tick), a.steps, C.byref(ms)) == 0
    parent.fs3_destroy(h)
    return ms.value / a.steps


def window(name, track, profile=False):
    if name == "parent":
        return parent_window()
    settings, off, tick = g.dam_break_3d(a.n)
    sim = g.FluidSimulation3D(settings, device=0, initial_offset=off, track=track)
    sim.timed_steps(tick, a.warmup)
    if profile:
        sim.profile(True)
        for _ in range(a.steps):
            sim.tick(tick)
        ms, steps = sim.profile_read()
        sim.close()
        return {p: round(m / steps, 4) for p, m in ms.items()}
    ms = sim.timed_steps(tick, a.steps) / a.steps
    sim.close()
    return ms


res = {"n": a.n, "warmup": a.warmup, "steps": a.steps}
for name, _ in SETTINGS:
    res[name + "_ms"] = []
k = len(SETTINGS)
for r in range(a.rounds):
    for name, track in SETTINGS[r % k:] + SETTINGS[:r % k]:
        res[name + "_ms"].append(round(window(name, track), 4))
for name, _ in SETTINGS:
    res[name + "_median_ms"] = statistics.median(res[name + "_ms"])
res["c0_minus_off_ms"] = round(res["c0_median_ms"] - res["off_median_ms"], 4)
res["c4_minus_off_ms"] = round(res["c4_median_ms"] - res["off_median_ms"], 4)
if parent is not None:
    res["parent_spread_ms"] = round(max(res["parent_ms"]) - min(res["parent_ms"]), 4)
    res["off_median_inside_parent_window"] = min(res["parent_ms"]) <= res["off_median_ms"] <= max(res["parent_ms"])
for name, track in SETTINGS:
    if name != "parent":
        res["passes_" + name + "_ms"] = window(name, track, profile=True)
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
