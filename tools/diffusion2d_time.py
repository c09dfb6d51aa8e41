"""The workload of DESIGN.md §27's cost table, to be run on the GPU:
  python tools/diffusion2d_time.py [n] [warm] [steps] [reps] [modes]
the dam_break_2d step (reference sort, IEEE) with four tracking channels in the modes `off` (tracking only), `d1` (one diffusing
channel), `d4` (four: two launches of two; with FS_DIFFUSE_SPLIT=0 in the environment one launch of four), `buoy` (a buoyancy channel and no
diffusing one: k_buoyancy), `d1buoy` (both: the tail of k_diffuse) and, not in the default list, `d1st` (one diffusing channel
with surface tension on, for a trace that holds k_diffuse beside k_surface_tension and k_density) — fresh handles, alternating, device events around the
window.  The conductivity is a quarter of FluidSimulation.diffusion_limit at the lattice's density, the channel values are the
particles' heights.  The pass alone comes from a kernel trace of the same command with one mode
(rocprofv3 --kernel-trace --stats -- python tools/diffusion2d_time.py 16777216 10 40 1 d1)."""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096 ** 2
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 10
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 100
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
modes = sys.argv[5].split(",") if len(sys.argv) > 5 else ["off", "d1", "d4", "buoy", "d1buoy"]
st, off, tick = g.dam_break_2d(n)
rho0 = 4.0 / (np.pi * st.smoothing_radius ** 2) * 10.0          # about ten neighbours' worth of W(0): the lattice's order of magnitude
kappa = 0.25 * g.FluidSimulation.diffusion_limit(st, tick, rho0)
for rep in range(reps):
    for mode in modes:
        sim = g.FluidSimulation(st, device=0, initial_offset=off, track=4, surface_tension=mode == "d1st")
        y = np.ascontiguousarray(sim.download_particles()["position"][:, 1])
        for c in range(4):
            sim.set_attribute(c, y)
        for c in range({"d1": 1, "d4": 4, "d1buoy": 1, "d1st": 1}.get(mode, 0)):
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
