"""Render a few frames of the dam break to PNG (visual validation on a headless GPU box).
  python tools/render_frames.py [n] [frames] [outdir] [--faucet[=k]] [--paddle] [--float] [--heat]
--faucet: a tap and an outflow on top of the dam break — every k steps (default 4) a line nozzle of 64 particles
under the ceiling pours downwards, and every k steps the particles in a box at the floor's right-hand end are removed; the handle
is created with room for the tap's particles (capacity = 2 n).
--paddle: a moving body on top of the dam break — a plate from ceiling to floor, 1.2 thick, that starts just right
of the block and pushes it against the -x wall at 3 m/s until a quarter of the block's width is left, then stands; its pose is
set before every step.
--float: a dynamic body — a square box of half the fluid's density released above the block falls into the dam
break; the handle's body loads are on and BodyDynamics2D integrates them on the host between the steps (one sync per step): the
fluid's impulses slow and turn it (the bodies' contact model hands over momentum where particles are pushed out of the box, it is
no pressure integral, so the box sinks, slower than it would fall), and the host stops it at the floor.  Prints the box's pose
with every frame.
--heat: a heated strip along the floor — channel 0 is a temperature that diffuses (a quarter of
FluidSimulation.diffusion_limit) and is the buoyancy channel (beta 0.5 against the reference 0); every 8 steps the particles
within two smoothing radii of the floor's middle half are set to 1.  The frame shows the temperature through the sampler
(sample_grid's channel sum over its Shepard weight) in red over the density in blue, and prints the channel's range."""
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g
faucet = next((a for a in sys.argv[1:] if a.startswith("--faucet")), None)
paddle = "--paddle" in sys.argv
floating = "--float" in sys.argv
heat = "--heat" in sys.argv
sys.argv = [a for a in sys.argv if not a.startswith("--faucet") and a not in ("--paddle", "--float", "--heat")]
every = int(faucet.split("=")[1]) if faucet and "=" in faucet else 4
n = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 16
frames = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 150, 400, 800]
outdir = sys.argv[3] if len(sys.argv) > 3 else "gpurun_out/frames"
os.makedirs(outdir, exist_ok=True)
st, off, tick = g.dam_break_2d(n)
sim = g.FluidSimulation(st, device=0, initial_offset=off, capacity=2 * n if faucet else 0, track=1 if heat else None)
sp, (sx, sy) = st.particle_spacing, (st.size.x, st.size.y)
if paddle:
    L = round(n ** 0.5) * sp
    plate = np.full((4, 8), 255, dtype=np.uint8)         # [H, W]: solid but the two end columns in x
    plate[:, [0, -1]] = 0
    body = sim.add_body_mask(plate, (1.2, sy))
    px, stop, u = np.float32(-sx / 2 + L + 0.7), np.float32(-sx / 2 + 0.25 * L), np.float32(-3.0)
if floating:
    L = round(n ** 0.5) * sp
    side = 0.125 * L
    box = np.full((8, 8), 255, dtype=np.uint8)           # solid but its rim: the field pushes out of every side
    box[[0, -1], :] = 0
    box[:, [0, -1]] = 0
    floater = sim.add_body_mask(box, (side, side))
    # half as dense as the fluid it displaces (one particle of mass tick.mass per sp^2)
    mass = 0.5 * tick.mass * (side / sp) ** 2
    dyn = g.BodyDynamics2D(mass, mass * side * side / 6.0, (-sx / 2 + 0.5 * L, sy / 2 - L - side), gravity=(tick.gravity.x, tick.gravity.y),
                           particle_mass=tick.mass)
    sim.enable_body_loads()
    sim.set_body_motion(floater, *dyn.motion())
if heat:
    h = st.smoothing_radius
    rho0 = 4.0 / (np.pi * h * h) * 10.0                  # about ten neighbours' worth of W(0)
    sim.set_diffusion(0, 0.25 * g.FluidSimulation.diffusion_limit(st, tick, rho0))
    sim.set_buoyancy(0, 0.5, 0.0)
done = 0
for f in frames:
    while done < f:
        if paddle:
            moving = px > stop
            sim.set_body_motion(body, (px, 0.0), velocity=(float(u) if moving else 0.0, 0.0))
            if moving:
                px = px + u * np.float32(tick.delta)
        if faucet and done % every == 0:
            if sim.particle_count + 64 <= sim.capacity:       # +y is down: the tap sits under the ceiling, right of the block
                sim.emit_nozzle((0.25 * sx, -0.45 * sy), (sp, 0.0), (0.0, sp), (0.0, 4.0), 64, 1)
            sim.remove_box((0.45 * sx, 0.4 * sy), (0.5 * sx, 0.5 * sy))
        if heat and done % 8 == 0:
            pos, temp = sim.download_particles()["position"], sim.attribute(0)
            temp[(pos[:, 1] > sy / 2 - 2 * h) & (np.abs(pos[:, 0]) < sx / 4)] = 1.0      # +y is down: the floor
            sim.set_attribute(0, temp)
        sim.tick(tick); done += 1
        if floating:
            dyn.advance(sim, floater, tick)
            if dyn.centre[1] > 0.5 * (sy - side):             # +y is down: the floor
                dyn.centre[1], dyn.velocity[1] = 0.5 * (sy - side), 0.0
                sim.set_body_motion(floater, *dyn.motion())
    img = sim.render_density(640, 400)
    if heat:
        smp, attr = sim.sample_grid(640, 400, attributes=True)
        w = smp["weight"]
        t = np.where(w > 0, attr[0] / np.where(w > 0, w, 1), 0.0).astype(np.float32)
        img = np.stack([np.clip(t, 0, 1), 0.2 * img[..., 3], (1 - np.clip(t, 0, 1)) * img[..., 3], img[..., 3]], axis=-1).astype(np.float32)
        a = sim.attribute(0)
        print("  temperature in", [float(a.min()), float(a.max())], "mean", float(a.mean()), flush=True)
    g.write_png(os.path.join(outdir, f"{'faucet' if faucet else 'paddle' if paddle else 'float' if floating else 'heat' if heat else 'dam'}_{n}_{f:05d}.png"), img)
    print("frame", f, "particles", sim.particle_count, "alpha coverage", float((img[..., 3] > 0.5).mean()), flush=True)
    if floating:
        print("  box centre", dyn.centre.tolist(), "angle", dyn.angle, "velocity", dyn.velocity.tolist(), flush=True)
