"""Many repetitions of one cheap count-changing call in one process: host time of each, median and deciles.
  python tools/count_calls_time.py <2d|3d> nothing [reps]   remove_box with a box that matches nothing: the flags and offsets
                                                            passes and the count's read-back; the state does not change
  python tools/count_calls_time.py <2d|3d> nozzle [reps]    one 4096-record nozzle emission + sync, back to back, no step between
2d: dam_break_2d at 4096^2, 3d: dam_break_3d at 200^3, ten steps first.  Another build of the library: through tools/with_lib.py."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g

dim, mode = sys.argv[1], sys.argv[2]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else (300 if mode == "nothing" else 60)
big = 1e6
if dim == "2d":
    n = 4096 * 4096
    st, off, tick = g.dam_break_2d(n)
    sim = g.FluidSimulation(st, device=0, initial_offset=off, capacity=n + 4096 * (reps + 2))
    lo, hi = (big, big), (2 * big, 2 * big)
    sp = st.particle_spacing
    emit = lambda: sim.emit_nozzle((0.0, -0.4 * st.size.y), (sp, 0.0), (0.0, sp), (0.0, 3.0), 4096, 1)
else:
    n = 200 ** 3
    st, off, tick = g.dam_break_3d(n)
    sim = g.FluidSimulation3D(st, device=0, initial_offset=off)
    sim.reserve(n + 4096 * (reps + 2))
    lo, hi = (big, big, big), (2 * big, 2 * big, 2 * big)
    sp = st.particle_spacing
    emit = lambda: sim.emit_nozzle((0.0, -0.4 * st.size.y, 0.0), (sp, 0.0, 0.0), (0.0, 0.0, sp), (0.0, 3.0, 0.0), 64, 64)
for _ in range(10):
    sim.tick(tick)
sim.sync()
ms = []
if mode == "nothing":
    sim.remove_box(lo, hi)
    for _ in range(reps):
        t0 = time.perf_counter()
        r = sim.remove_box(lo, hi)
        ms.append((time.perf_counter() - t0) * 1e3)
        assert r == 0
else:
    emit(); sim.sync()                     # loads the kernel; in 2D it also crosses 2^24
    for _ in range(reps):
        t0 = time.perf_counter()
        emit(); sim.sync()
        ms.append((time.perf_counter() - t0) * 1e3)
ms = np.array(ms)
print(f"{dim} {mode} x{reps}: median {np.median(ms):.4f} p10 {np.quantile(ms, 0.1):.4f} p90 {np.quantile(ms, 0.9):.4f} ms (count now {sim.particle_count})", flush=True)
sim.close()
