"""Render a few frames of the 3D dam break to PNG through the ray-marched G-buffer, headless:
  python tools/render_frames3d.py [n] [frame,frame,...] [outdir] [width] [height] [--box x0,y0,z0,x1,y1,z1[,voxels]]
                                  [--surface-tension SIGMA[,TAU]] [--dye] [--faucet K[,NU,NV]] [--paddle [AMPLITUDE,PERIOD]] [--float]
                                  [--heat [BETA]]
--heat: one tracking channel is a temperature.  A patch of the floor (+y) under the middle of the initial block, a
third of the block's side wide, holds the particles within 2 h of it at 1.0 (re-applied every tenth step from a download of the
positions); the channel diffuses at a quarter of FluidSimulation3D.diffusion_limit and is the buoyancy channel with expansion
coefficient BETA (default 0.5) about 0.0, so the warm fluid rises as a plume.  The shaded surface is tinted red by the channel's
Shepard value at the hit points (sample_attr), as with --dye.
--float: a dynamic body — a cube of half the fluid's density, a quarter of the block's side, released above the
block falls onto the dam break; the handle's body loads are on and BodyDynamics3D integrates them on the host between the steps
(one sync per step): the fluid's impulses slow and turn it (the bodies' contact model hands over momentum where particles are
pushed out of the box, it is no pressure integral), and the host stops it at the floor.  Prints the box's pose with every frame;
the box itself is not drawn.
--paddle: a moving rigid body: a plate across the tank, as high and deep as the box and 3 h thick, that swings along
x about the middle of the tank, x(t) = AMPLITUDE * sin(2 pi t / PERIOD) (default a twentieth of the box's width, 2 s); its pose and
velocity are set before every step.  The dam breaks against it and it keeps making waves; the plate itself is not drawn.
--faucet: a particle count that grows: the handle reserves room for twice its particles and a nozzle under the
ceiling, above the dry half of the tank, emits a layer of NU x NV particles (default 16 x 16, one spacing apart, falling at 3 m/s)
every K steps until the capacity is reached.  With --box the jet fills a tank that has an obstacle in it.
--dye: particle tracking with one channel: the particles of the -x half of the initial block carry 1.0, the others
0.0; the shaded surface is tinted red by the Shepard value of the channel at the hit points (sampled there with sample_attr).
--surface-tension: the opt-in colour-field surface tension with coefficient SIGMA and threshold TAU (default 1.0).
--box: a static obstacle, a box in world coordinates (+y is the floor) rasterised to a mask of `voxels` (default
64) voxels along x and as many along y and z as keep them near cubes; the fluid flows around it, the box itself is not drawn."""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g
box = None
if "--box" in sys.argv:
    k = sys.argv.index("--box")
    box = [float(x) for x in sys.argv[k + 1].split(",")]
    del sys.argv[k:k + 2]
tension = None
if "--surface-tension" in sys.argv:
    k = sys.argv.index("--surface-tension")
    tension = [float(x) for x in sys.argv[k + 1].split(",")]
    del sys.argv[k:k + 2]
faucet = None
if "--faucet" in sys.argv:
    k = sys.argv.index("--faucet")
    faucet = [int(x) for x in sys.argv[k + 1].split(",")]
    faucet = (faucet + [16, 16])[:3] if len(faucet) == 1 else faucet
    del sys.argv[k:k + 2]
paddle = None
if "--paddle" in sys.argv:
    k = sys.argv.index("--paddle")
    given = k + 1 < len(sys.argv) and "," in sys.argv[k + 1]
    paddle = [float(x) for x in sys.argv[k + 1].split(",")] if given else []
    del sys.argv[k:k + (2 if given else 1)]
floating = "--float" in sys.argv
if floating:
    sys.argv.remove("--float")
heat = None
if "--heat" in sys.argv:
    k = sys.argv.index("--heat")
    try:                                            # BETA is written with a point: "--heat 64000" is a particle count
        given = "." in sys.argv[k + 1] and np.isfinite(float(sys.argv[k + 1]))
    except (IndexError, ValueError):
        given = False
    heat = float(sys.argv[k + 1]) if given else 0.5
    del sys.argv[k:k + (2 if given else 1)]
dye = "--dye" in sys.argv
if dye:
    sys.argv.remove("--dye")
n = int(sys.argv[1]) if len(sys.argv) > 1 else 64 ** 3
frames = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 60, 150, 300]
outdir = sys.argv[3] if len(sys.argv) > 3 else "build/frames3d"
width = int(sys.argv[4]) if len(sys.argv) > 4 else 640
height = int(sys.argv[5]) if len(sys.argv) > 5 else 400
os.makedirs(outdir, exist_ok=True)
st, off, tick = g.dam_break_3d(n)
sim = g.FluidSimulation3D(st, device=0, initial_offset=off)
sx, sy, sz = st.size.x, st.size.y, st.size.z
if box is not None:
    w = int(box[6]) if len(box) > 6 else 64
    shape = (w, max(1, round(w * sy / sx)), max(1, round(w * sz / sx)))
    sim.set_collider_mask(g.box_mask3d((sx, sy, sz), shape, box[0:3], box[3:6]))
    print("collider", sim.collider_dims, flush=True)
if paddle is not None:
    amp, period = paddle if paddle else (0.05 * sx, 2.0)
    mask = np.full((1, 1, 5), 255, dtype=np.uint8)      # five slices along x, solid but the two end slices
    mask[:, :, [0, -1]] = 0
    plate = sim.add_body_mask(mask, (5 * st.smoothing_radius, sy, sz))
    print("paddle: body", plate, sim.body_dims(plate), "amplitude", amp, "period", period, flush=True)
if floating:
    sp = st.particle_spacing
    L = round(n ** (1.0 / 3.0)) * sp
    side = 0.25 * L
    cube = np.full((8, 8, 8), 255, dtype=np.uint8)       # solid but its rim: the field pushes out of every face
    for axis in range(3):
        rim = [slice(None)] * 3
        rim[axis] = [0, -1]
        cube[tuple(rim)] = 0
    floater = sim.add_body_mask(cube, (side, side, side))
    mass = 0.5 * tick.mass * (side / sp) ** 3            # half as dense as the fluid it displaces (one particle per sp^3)
    inertia = mass * side * side / 6.0
    dyn = g.BodyDynamics3D(mass, (inertia, inertia, inertia), (-sx / 2 + 0.5 * L + 0.5 * sp, sy / 2 - L - side, 0.0),
                           gravity=(tick.gravity.x, tick.gravity.y, tick.gravity.z), particle_mass=tick.mass)
    sim.enable_body_loads()
    sim.set_body_motion(floater, *dyn.motion())
    print("float: body", floater, sim.body_dims(floater), "mass", mass, flush=True)
if tension is not None:
    sim.set_surface_tension(tension[0], tension[1] if len(tension) > 1 else 1.0)
    print("surface tension", sim.surface_tension_params, flush=True)
if dye:
    x0 = sim.download_particles()["position"][:, 0]
    sim.track(1)                                    # ids = the slots of this download
    sim.set_attribute(0, (x0 < np.median(x0)).astype(np.float32))
if heat is not None:
    L = round(n ** (1.0 / 3.0)) * st.particle_spacing
    patch_x, patch_half = -sx / 2 + 0.5 * L, L / 6.0

    def reheat():
        p = sim.download_particles()["position"]
        a = sim.attribute(0)
        hot = (p[:, 1] > sy / 2 - 2 * st.smoothing_radius) & (np.abs(p[:, 0] - patch_x) < patch_half) & (np.abs(p[:, 2]) < patch_half)
        a[hot] = 1.0
        sim.set_attribute(0, a)
        return int(hot.sum())
    sim.track(1)
    sim.tick(tick)                                     # densities exist after a step
    rho0 = float(np.median(sim.download_particles()["density"]))
    sim.set_diffusion(0, 0.25 * g.FluidSimulation3D.diffusion_limit(st, tick, rho0))
    sim.set_buoyancy(0, heat, 0.0)
    print("heat: conductivity", sim.diffusion(0), "buoyancy", sim.buoyancy, "hot particles", reheat(), flush=True)
# gravity is +y: "up" is -y.  From in front of the -z wall, above the floor, looking at the middle of the tank.
eye = (-0.15 * sx, -0.55 * sy, -0.5 * sz - 0.9 * sx)
cam = g.look_at_camera(eye, (0.0, 0.15 * sy, 0.0), (0.0, -1.0, 0.0), np.radians(42.0), width, height)
h = st.smoothing_radius
if faucet is not None:
    sim.reserve(2 * n)
    sp = st.particle_spacing
    nozzle = dict(origin=(0.25 * sx, -0.5 * sy + 2 * h, 0.0), u=(sp, 0.0, 0.0), v=(0.0, 0.0, sp), velocity=(0.0, 3.0, 0.0),
                  nu=faucet[1], nv=faucet[2])
done = 1 if heat is not None else 0
for f in frames:
    while done < f:
        if faucet is not None and done % faucet[0] == 0 and sim.particle_count + faucet[1] * faucet[2] <= sim.capacity:
            sim.emit_nozzle(**nozzle)
        if paddle is not None:
            om = 2.0 * np.pi / period
            t = (done + 1) * tick.delta                 # the pose at the end of the step that is about to run
            sim.set_body_motion(plate, (amp * np.sin(om * t), 0.0, 0.0), velocity=(amp * om * np.cos(om * t), 0.0, 0.0))
        sim.tick(tick); done += 1
        if heat is not None and done % 10 == 0:
            reheat()
        if floating:
            dyn.advance(sim, floater, tick)
            if dyn.centre[1] > 0.5 * (sy - side):           # +y is down: the floor
                dyn.centre[1], dyn.velocity[1] = 0.5 * (sy - side), 0.0
                sim.set_body_motion(floater, *dyn.motion())
    if faucet is not None:
        print("frame", f, "particles", sim.particle_count, "of", sim.capacity, flush=True)
    iso = 0.5 * float(np.median(sim.download_particles()["density"]))
    reach = 1.2 * (abs(eye[2]) + 0.5 * sz) + sx
    hits = sim.render_surface(cam, g.SurfaceParams3(iso, 0.0, 0.5 * h, min(4096, int(reach / (0.5 * h)) + 1), 8))
    rgba = g.shade_surface(hits, max_speed=6.0)[::-1]                 # row 0 of the G-buffer is the image's bottom edge
    if dye or heat is not None:                     # visual only: the channel's Shepard value where the rays hit
        lit = hits["hit"] != 0
        wgt, sums = sim.sample_attr(g.surface_hit_points(cam, hits)[lit], weights=True)
        c = np.zeros(hits.shape, dtype=np.float32)
        c[lit] = np.where(wgt > 0, sums[0] / np.where(wgt > 0, wgt, 1), 0)
        c = c[::-1, :, None]
        print("frame", f, "mean temperature of the hits" if heat is not None else "dyed share of the hits", round(float(c[rgba[..., 3] > 0].mean()), 4),
              "max", round(float(c.max()), 4), flush=True)
        if heat is not None:                        # what reaches the surface has diffused: show a tenth of the patch's value as full red
            c = np.clip(c * 10.0, 0.0, 1.0)
        shade = rgba[..., :3].max(axis=-1, keepdims=True)
        rgba[..., :3] = rgba[..., :3] * (1 - c) + np.float32([0.9, 0.15, 0.1]) * shade * c
    g.write_png(os.path.join(outdir, f"dam3d_{n}_{f:05d}.png"), rgba, background=(0.04, 0.04, 0.06))
    print("frame", f, "coverage", round(float((hits["hit"] != 0).mean()), 4), "mean march index of hits",
          round(float(hits["steps"][hits["hit"] != 0].mean()), 1), flush=True)
    if floating:
        print("  box centre", dyn.centre.tolist(), "velocity", dyn.velocity.tolist(), "angular velocity", dyn.angular_velocity.tolist(), flush=True)
sim.close()
