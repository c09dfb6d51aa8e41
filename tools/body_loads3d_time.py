"""The workload of DESIGN.md §26's cost table, to be run on the GPU:
  python tools/body_loads3d_time.py [n] [warm] [steps] [reps] [scenes] [modes]
the dam_break_3d step (IEEE) with three scenes — `dry1`: one body outside the domain, which touches nothing; `dry8`: eight such
bodies; `paddle`: the paddle of tools/bodies3d_time.py in the fluid, hit every step — each with the handle's body loads off and on
(modes: off, on or both; fresh handles, alternating, device events around the window).  Prints the step time and, with loads on,
the paddle's words over the window.  The bodies' pass alone (k3_bodies with loads off, k3_bodies_loads + k3_body_loads_fold with
loads on) comes from a kernel trace of the same command with one scene and one mode
(rocprofv3 --kernel-trace --stats -- python tools/body_loads3d_time.py 8000000 10 40 1 paddle on)."""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200 ** 3
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 10
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 100
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
scenes = sys.argv[5].split(",") if len(sys.argv) > 5 else ["dry1", "dry8", "paddle"]
modes = {"off": [False], "on": [True], "both": [False, True]}[sys.argv[6] if len(sys.argv) > 6 else "both"]
st, off, tick = g.dam_break_3d(n)
sx, sy, sz = st.size.x, st.size.y, st.size.z
L = round(n ** (1.0 / 3.0)) * st.particle_spacing
plate = np.full((4, 4, 8), 255, dtype=np.uint8)          # [D, H, W]: solid but the two end slices in x
plate[:, :, [0, -1]] = 0
u = np.float32(-1.5)
for rep in range(reps):
    for scene in scenes:
        for on in modes:
            sim = g.FluidSimulation3D(st, device=0, initial_offset=off)
            count = 8 if scene == "dry8" else 1
            for slot in range(count):
                sim.add_body_mask(plate, (0.3, sy, sz))
                sim.set_body_motion(slot, (3.0 * sx, 0.0, 0.0))      # outside the domain
            if on:
                sim.enable_body_loads()
            c = np.array([-sx / 2 + L + 0.1, 0.0, 0.0], dtype=np.float32)
            for _ in range(warm):
                if scene == "paddle":
                    c = c + np.array([u * np.float32(tick.delta), 0, 0], dtype=np.float32)
                    sim.set_body_motion(0, c, velocity=(float(u), 0.0, 0.0))
                sim.tick(tick)
            if on:
                sim.body_loads(0, reset=True)
            sim.sync()
            ms = sim.timed_steps(tick, steps) / steps
            line = f"step n={n} {scene} loads {'on' if on else 'off'} rep {rep}: {ms:.4f} ms/step (steps {warm}-{warm + steps})"
            if on:
                r = sim.body_loads(0)
                line += (f"; body 0: hits/step {r.hits / max(r.steps, 1):.0f} dropped {r.dropped} mean force per unit mass "
                         f"{r.mean_force(1.0, tick.delta).tolist()} mean torque {r.mean_torque(1.0, tick.delta).tolist()}")
            print(line, flush=True)
            sim.close()
