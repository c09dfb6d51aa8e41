"""The workload of DESIGN.md §18's cost table, to be run on the GPU:
  python tools/collide3d_time.py [n] [warm] [steps] [reps]
the dam_break_3d step without a collider and with a 64^3 box collider (both math modes, fresh handles, alternating, device events
around the window), and the blocking producer call at 64^3 and 256^3 (host clock around fs3_collider_from_mask, mask copy included)."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200 ** 3
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 10
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 100
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
st, off, tick = g.dam_break_3d(n)
size = (st.size.x, st.size.y, st.size.z)
# a box on the floor (+y) right of the initial block, across the depth: the dam runs into it inside the timed window
lo = (0.05 * size[0], size[1] / 2 - 0.3 * size[1], -size[2] / 2)
hi = (0.15 * size[0], size[1] / 2, size[2] / 2)
mask64 = g.box_mask3d(size, (64, 64, 64), lo, hi)
for mode, name in ((g.FS_MATH_IEEE, "strict"), (g.FS_MATH_TOLERANCE, "tolerance")):
    for rep in range(reps):
        for collider in (False, True):
            sim = g.FluidSimulation3D(st, device=0, initial_offset=off, math_mode=mode)
            if collider:
                sim.set_collider_mask(mask64)
            for _ in range(warm):
                sim.tick(tick)
            sim.sync()
            ms = sim.timed_steps(tick, steps) / steps
            sim.profile(True); sim.profile_read(True)
            sim.timed_steps(tick, 20)
            p, k = sim.profile_read(True)
            x = sim.download_particles()["position"][:, 0]
            print(f"step {name} n={n} collider={'64^3 box' if collider else 'none'} rep {rep}: {ms:.4f} ms/step (steps {warm}-{warm + steps}); "
                  f"force pass of the next 20 steps {p['force'] / k:.4f} ms; particles past the box's near face {int((x > lo[0]).sum())}", flush=True)
            sim.close()
sim = g.FluidSimulation3D(*g.dam_break_3d(16 ** 3)[:1], device=0)
for w in (64, 256):
    mask = g.box_mask3d(size, (w, w, w), lo, hi)
    sim.set_collider_mask(mask)                      # warm-up: code objects, the first allocation
    ts = []
    for _ in range(5):
        t0 = time.perf_counter(); sim.set_collider_mask(mask); ts.append((time.perf_counter() - t0) * 1e3)
    print(f"producer {w}^3 box mask, blocking call: min {min(ts):.3f} ms, median {sorted(ts)[2]:.3f} ms, max {max(ts):.3f} ms", flush=True)
sim.close()
