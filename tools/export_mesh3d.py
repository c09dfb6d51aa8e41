"""Export the iso-surface of a few steps of the 3D dam break as Wavefront OBJ meshes (surface nets), headless:
  python tools/export_mesh3d.py [n] [step,step,...] [outdir] [nodes along x]"""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g
n = int(sys.argv[1]) if len(sys.argv) > 1 else 64 ** 3
steps = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 60, 150, 300]
outdir = sys.argv[3] if len(sys.argv) > 3 else "build/mesh3d"
nx = int(sys.argv[4]) if len(sys.argv) > 4 else 192
os.makedirs(outdir, exist_ok=True)
st, off, tick = g.dam_break_3d(n)
sim = g.FluidSimulation3D(st, device=0, initial_offset=off)
h = st.smoothing_radius
# the whole domain and h more on every side, so the mesh is closed; cubic voxels
lo = np.float64([-st.size.x / 2, -st.size.y / 2, -st.size.z / 2]) - h
hi = -lo
dims = [max(2, int(round(nx * (hi[a] - lo[a]) / (hi[0] - lo[0])))) for a in range(3)]
done = 0
for s in steps:
    while done < s:
        sim.tick(tick); done += 1
    iso = 0.5 * float(np.median(sim.download_particles()["density"]))
    verts, tris = sim.extract_surface(dims[0], dims[1], dims[2], iso, tuple(lo), tuple(hi))
    path = os.path.join(outdir, f"dam3d_{n}_{s:05d}.obj")
    g.write_obj(path, verts, tris)
    print("step", s, "lattice", dims, "vertices", verts.shape[0], "triangles", tris.shape[0], "->", path, flush=True)
sim.close()
