"""What the opt-in particle tracking costs: the 16 M dam break over bench.py's window (10 warm-up + 100 timed
steps, from a fresh handle) with tracking off, with ids only (C = 0) and with four channels (C = 4), alternated, each round
starting with another setting; then one window per setting with pass events (the carry pass falls inside the reorder interval).

  python tools/ab_track.py [--n N] [--rounds R] [--warmup W] [--steps K] [--out FILE]

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
ap.add_argument("--n", type=int, default=1 << 24)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--out", default=None)
a = ap.parse_args()

SETTINGS = (("off", None), ("c0", 0), ("c4", 4))


def window(track, profile=False):
    settings, off, tick = g.dam_break_2d(a.n)
    sim = g.FluidSimulation(settings, device=0, initial_offset=off, track=track)
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
for r in range(a.rounds):
    order = SETTINGS[r % 3:] + SETTINGS[:r % 3]
    for name, track in order:
        res[name + "_ms"].append(round(window(track), 4))
for name, _ in SETTINGS:
    res[name + "_median_ms"] = statistics.median(res[name + "_ms"])
res["c0_minus_off_ms"] = round(res["c0_median_ms"] - res["off_median_ms"], 4)
res["c4_minus_off_ms"] = round(res["c4_median_ms"] - res["off_median_ms"], 4)
for name, track in SETTINGS:
    res["passes_" + name + "_ms"] = window(track, profile=True)
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
