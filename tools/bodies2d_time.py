"""The workload of DESIGN.md §24's cost table, to be run on the GPU:
  python tools/bodies2d_time.py [n] [warm] [steps] [reps] [sorts] [counts] [dry]
the dam_break_2d step with 0, 1 and 8 moving bodies (fresh handles, alternating, device events around the window; sorts: bitonic,
counting or both; counts: which of 0,1,8, e.g. 8 alone under a kernel trace).  The counterpart of tools/bodies3d_time.py.
Body 0 is the paddle of tools/render_frames.py --paddle: a plate from ceiling to floor, 1.2 thick, that starts inside the initial
block and is driven towards the -x wall at 3 m/s, its pose set before every warm-up step; through the timed window it stands
where the warm-up left it (fs_timed_steps enqueues its steps without returning to the host) and keeps its velocity, so the fluid
in it is hit every step.  Bodies 1 .. 7 are thin plates spread over the dry half of the tank, turned (at 16 M the wave does not
reach them within 110 steps: they cost their box tests).
With `dry` as the last argument every body stands outside the domain instead: no particle passes a box test, the steps compute
the bits of a handle without bodies, and what the step gains over bodies=0 is the pass alone — in the wet scene the paddle also
changes the flow, and with it the cost of the density and force passes.
Prints the step time and how many particles lie inside a body's box at the end; k_bodies alone comes from a kernel trace of the
same command (rocprofv3 --kernel-trace --stats -- python tools/bodies2d_time.py 16777216 10 40 1 bitonic 8)."""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096 ** 2
warm = int(sys.argv[2]) if len(sys.argv) > 2 else 10
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 100
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 3
sorts = sys.argv[5] if len(sys.argv) > 5 else "bitonic"
counts = [int(x) for x in sys.argv[6].split(",")] if len(sys.argv) > 6 else [0, 1, 8]
dry = len(sys.argv) > 7 and sys.argv[7] == "dry"
st, off, tick = g.dam_break_2d(n)
sx, sy = st.size.x, st.size.y
L = round(n ** 0.5) * st.particle_spacing
plate = np.full((4, 8), 255, dtype=np.uint8)             # [H, W]: solid but the two end columns in x
plate[:, [0, -1]] = 0
u = np.float32(-3.0)


def add_bodies(sim, count):
    """-> the boxes (centre, rot[2, 2], half extent) for the census at the end"""
    boxes = []
    if count >= 1:
        sim.add_body_mask(plate, (1.2, sy))
        boxes.append([np.array([-sx / 2 + 0.5 * L, 0.0], dtype=np.float32), np.eye(2), np.array([0.6, sy / 2])])
    for k in range(1, count):
        slot = sim.add_body_mask(plate, (1.2, 0.5 * sy))
        c, rot = g.rigid_motion2d((0.05 * sx + (k - 1) * 0.06 * sx, 0.25 * sy), (0, 0), 0.2 * k, 1.0)
        sim.set_body_motion(slot, c, rot)
        boxes.append([c, rot.reshape(2, 2).astype(np.float64), np.array([0.6, 0.25 * sy])])
    return boxes


for sort, name in ((g.FS_SORT_BITONIC, "bitonic"), (g.FS_SORT_COUNTING, "counting")):
    if sorts not in ("both", name):
        continue
    for rep in range(reps):
        for count in counts:
            sim = g.FluidSimulation(st, device=0, initial_offset=off, sort_mode=sort)
            boxes = add_bodies(sim, count)
            for slot in range(count if dry else 0):
                boxes[slot][0] = np.array([3.0 * sx, 0.0], dtype=np.float32)
                sim.set_body_motion(slot, boxes[slot][0], boxes[slot][1].reshape(4))
            for _ in range(warm):
                if count and not dry:
                    boxes[0][0] = boxes[0][0] + np.array([u * np.float32(tick.delta), 0], dtype=np.float32)
                    sim.set_body_motion(0, boxes[0][0], velocity=(float(u), 0.0))
                sim.tick(tick)
            sim.sync()
            ms = sim.timed_steps(tick, steps) / steps
            pos = sim.download_particles()["position"].astype(np.float64)
            inside = np.zeros(pos.shape[0], dtype=bool)
            for c, rot, hb in boxes:
                inside |= (np.abs((pos - c) @ rot) <= hb).all(axis=1)
            print(f"step {name} n={n} bodies={count}{' dry' if dry else ''} rep {rep}: "
                  f"{ms:.4f} ms/step (steps {warm}-{warm + steps}); particles inside a body's box {int(inside.sum())}", flush=True)
            sim.close()
