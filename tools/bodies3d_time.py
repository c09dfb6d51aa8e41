"""The workload of DESIGN.md §23's cost table, to be run on the GPU:
  python tools/bodies3d_time.py [n] [warm] [steps] [reps] [modes] [counts] [dry]
the dam_break_3d step with 0, 1 and 8 moving bodies (fresh handles, alternating, device events around the window; modes: strict,
tolerance or both; counts: which of 0,1,8, e.g. 8 alone under a kernel trace).
Body 0 is the paddle of tests/bodies3d_ref.py scaled to the box: a plate across the tank, 0.3 thick, that starts one particle
spacing right of the initial block and is driven into it at 1.5 m/s, its pose set before every warm-up step; through the timed
window it stands where the warm-up left it (fs3_timed_steps enqueues its steps without returning to the host) and keeps its
velocity, so the fluid pressed against it is hit every step.  Bodies 1 .. 7 are thin plates spread over the dry half of the tank,
turned about z (at 8 M the wave does not reach them within 110 steps: they cost their box tests).
With `dry` as the last argument every body stands outside the domain instead: no particle passes a box test, the steps compute
the bits of a handle without bodies, and what the step gains over bodies=0 is the pass alone — in the wet scene the paddle also
changes the flow, and with it the cost of the density and force passes.
Prints the step time and how many particles lie inside a body's box at the end; k3_bodies alone comes from a kernel trace of the
same command (rocprofv3 --kernel-trace --stats -- python tools/bodies3d_time.py 8000000 10 40 1 strict 8)."""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g
n = int(sys.argv[1]) if len(sys.argv) > 1 else 200 ** 3
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 10
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 100
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
modes = sys.argv[5] if len(sys.argv) > 5 else "both"
counts = [int(x) for x in sys.argv[6].split(",")] if len(sys.argv) > 6 else [0, 1, 8]
dry = len(sys.argv) > 7 and sys.argv[7] == "dry"
st, off, tick = g.dam_break_3d(n)
sx, sy, sz = st.size.x, st.size.y, st.size.z
L = round(n ** (1.0 / 3.0)) * st.particle_spacing
plate = np.full((4, 4, 8), 255, dtype=np.uint8)          # [D, H, W]: solid but the two end slices in x
plate[:, :, [0, -1]] = 0
u = np.float32(-1.5)


def add_bodies(sim, count):
    """-> the boxes (centre, rot[3, 3], half extent) for the census at the end"""
    boxes = []
    if count >= 1:
        sim.add_body_mask(plate, (0.3, sy, sz))
        boxes.append([np.array([-sx / 2 + L + 0.1, 0.0, 0.0], dtype=np.float32), np.eye(3), np.array([0.15, sy / 2, sz / 2])])
    for k in range(1, count):
        slot = sim.add_body_mask(plate, (0.3, 0.5 * sy, sz))
        c, rot = g.rigid_motion((0.05 * sx + (k - 1) * 0.06 * sx, 0.25 * sy, 0.0), (0, 0, 0), (0, 0, 1), 0.2 * k, 1.0)
        sim.set_body_motion(slot, c, rot)
        boxes.append([c, rot.reshape(3, 3).astype(np.float64), np.array([0.15, 0.25 * sy, sz / 2])])
    return boxes


for mode, name in ((g.FS_MATH_IEEE, "strict"), (g.FS_MATH_TOLERANCE, "tolerance")):
    if modes not in ("both", name):
        continue
    for rep in range(reps):
        for count in counts:
            sim = g.FluidSimulation3D(st, device=0, initial_offset=off, math_mode=mode)
            boxes = add_bodies(sim, count)
            for slot in range(count if dry else 0):
                boxes[slot][0] = np.array([3.0 * sx, 0.0, 0.0], dtype=np.float32)
                sim.set_body_motion(slot, boxes[slot][0], boxes[slot][1].reshape(9))
            for _ in range(warm):
                if count and not dry:
                    boxes[0][0] = boxes[0][0] + np.array([u * np.float32(tick.delta), 0, 0], dtype=np.float32)
                    sim.set_body_motion(0, boxes[0][0], velocity=(float(u), 0.0, 0.0))
                sim.tick(tick)
            sim.sync()
            ms = sim.timed_steps(tick, steps) / steps
            pos = sim.download_particles()["position"].astype(np.float64)
            inside = np.zeros(pos.shape[0], dtype=bool)
            for c, rot, hb in boxes:
                inside |= (np.abs((pos - c) @ rot) <= hb).all(axis=1)
            print(f"step {name} n={n} bodies={count}{' dry' if dry else ''} rep {rep}: {ms:.4f} ms/step (steps {warm}-{warm + steps}); "
                  f"particles inside a body's box {int(inside.sum())}", flush=True)
            sim.close()
