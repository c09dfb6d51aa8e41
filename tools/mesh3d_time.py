"""The workload of DESIGN.md §17's timing table: dam_break_3d at n particles after `steps` steps, one surface extraction on an
N^3 node lattice over the domain and one fs3_sample_grid of the same view (the only other route to the node field).  Run it
under a kernel trace and read the per-kernel device times from the trace's statistics:
  python tools/mesh3d_time.py [n] [steps] [N]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g
n = int(sys.argv[1]) if len(sys.argv) > 1 else 100 ** 3
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
N = int(sys.argv[3]) if len(sys.argv) > 3 else 256
st, off, tick = g.dam_break_3d(n)
sim = g.FluidSimulation3D(st, device=0, initial_offset=off)
sim.timed_steps(tick, steps)
iso = 0.5 * float(np.median(sim.download_particles()["density"]))
for rep in range(2):                                   # the first call allocates the scratch
    t0 = time.perf_counter()
    verts, tris = sim.extract_surface(N, N, N, iso)
    t1 = time.perf_counter()
    print("extract_surface", N, "vertices", verts.shape[0], "triangles", tris.shape[0], "host ms", round(1e3 * (t1 - t0), 2), flush=True)
t0 = time.perf_counter()
vol = sim.sample_grid(N, N, N)
print("sample_grid", N, "host ms", round(1e3 * (time.perf_counter() - t0), 2), "nodes inside", int((vol["density"] >= np.float32(iso)).sum()), flush=True)
sim.close()
