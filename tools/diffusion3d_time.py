"""The workload of DESIGN.md §28's cost table, to be run on the GPU:
  python tools/diffusion3d_time.py [n] [warm] [steps] [reps] [modes]
the dam_break_3d step (IEEE) with four tracking channels in the modes `off` (tracking only), `d1` (one diffusing channel:
k3_diffuse<1>), `d2` (two: one launch of k3_diffuse<2>), `d4` (four: two launches of two), `buoy` (a buoyancy channel and no
diffusing one: k3_buoyancy), `d1buoy` (both: the tail of k3_diffuse<1>) and, not in the default list, `d1st` / `d2st` (with surface
tension on, for a trace that holds k3_diffuse beside k3_surface_tension and k3_density) — fresh handles, alternating, device events
around the window.  The conductivity is a quarter of FluidSimulation3D.diffusion_limit at the lattice's density, the channel values
are the particles' heights.  The pass alone and the row copy come from a kernel trace of the same command with one mode
(rocprofv3 --kernel-trace --memory-copy-trace --stats -- python tools/diffusion3d_time.py 8000000 10 40 1 d1st)."""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200 ** 3
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 10
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 100
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
modes = sys.argv[5].split(",") if len(sys.argv) > 5 else ["off", "d1", "d2", "d4", "buoy", "d1buoy"]
st, off, tick = g.dam_break_3d(n)
h, s = st.smoothing_radius, st.particle_spacing
rho0 = 315.0 / (64.0 * np.pi * h ** 9) * (h * h) ** 3 * (4.0 / 3.0 * np.pi * (h / s) ** 3) * 0.3      # ~33 neighbours at a third of W(0)
kappa = 0.25 * g.FluidSimulation3D.diffusion_limit(st, tick, rho0)
for rep in range(reps):
    for mode in modes:
        sim = g.FluidSimulation3D(st, device=0, initial_offset=off, track=4)
        if mode.endswith("st"):
            sim.set_surface_tension(0.05, 0.1)
        y = np.ascontiguousarray(sim.download_particles()["position"][:, 1])
        for c in range(4):
            sim.set_attribute(c, y)
        for c in range({"d1": 1, "d2": 2, "d4": 4, "d1buoy": 1, "d1st": 1, "d2st": 2}.get(mode, 0)):
            sim.set_diffusion(c, kappa)
        if mode in ("buoy", "d1buoy"):
            sim.set_buoyancy(0, 0.01, float(y.mean()))
        for _ in range(warm):
            sim.tick(tick)
        sim.sync()
        ms = sim.timed_steps(tick, steps) / steps
        a = sim.attribute(0)
        print(f"step n={n} {mode} rep {rep}: {ms:.4f} ms/step (steps {warm}-{warm + steps}); channel 0 in [{a.min():.4f}, {a.max():.4f}]", flush=True)
        sim.close()
