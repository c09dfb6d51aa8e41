"""What the opt-in 3D surface tension costs: the 8 M 3D dam break over bench.py's window (10 warm-up + 100 timed
steps, from a fresh handle) with surface tension off and on, alternated, each round starting with the other setting; then one
window per setting with pass events (the ST pass falls inside the force interval).

  python tools/ab_surface_tension3d.py [--side S] [--rounds R] [--warmup W] [--steps K] [--sigma X] [--tau Y] [--tolerance] [--out FILE]

Prints one JSON object (also written to --out): ms per step of every window, the medians, the per-pass times.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=200)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--sigma", type=float, default=100.0)
ap.add_argument("--tau", type=float, default=1.7)
ap.add_argument("--tolerance", action="store_true")
ap.add_argument("--out", default=None)
a = ap.parse_args()
mode = g.FS_MATH_TOLERANCE if a.tolerance else g.FS_MATH_IEEE


def window(st_on, profile=False):
    settings, off, tick = g.dam_break_3d(a.side ** 3)
    sim = g.FluidSimulation3D(settings, device=0, initial_offset=off, math_mode=mode)
    if st_on:
        sim.set_surface_tension(a.sigma, a.tau)
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


res = {"side": a.side, "mode": "tolerance" if a.tolerance else "strict", "warmup": a.warmup, "steps": a.steps,
       "sigma": a.sigma, "tau": a.tau, "off_ms": [], "on_ms": []}
for r in range(a.rounds):
    for st_on in ((False, True) if r % 2 == 0 else (True, False)):
        res["on_ms" if st_on else "off_ms"].append(round(window(st_on), 4))
res["off_median_ms"] = statistics.median(res["off_ms"])
res["on_median_ms"] = statistics.median(res["on_ms"])
res["on_minus_off_ms"] = round(res["on_median_ms"] - res["off_median_ms"], 4)
res["passes_off_ms"] = window(False, profile=True)
res["passes_on_ms"] = window(True, profile=True)
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
