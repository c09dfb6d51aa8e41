"""What 3D surface rendering costs: the 8 M dam_break_3d scene after its window (10 warm-up + 100 steps), then a
1024^2 orthographic and a 1024^2 perspective view of the fluid, each timed two ways between a hipEvent pair on the simulation's
stream, in alternated windows, medians reported:
  fused     fs3_render_surface_device: one launch of k3_render_surface per image
  baseline  the same march with what the library offered before: one fs3_sample_points_device launch per march step k over ALL
            pixels (then one per bisection step and one at the hit), torch computing the points and keeping the hit mask
and against k3_density of the same run (the density pass of the profiled 100-step window).  The two G-buffers are compared:
`steps` and `hit` must agree exactly (torch's point arithmetic may contract, so t and the records are compared with a tolerance
and reported, not asserted bit for bit; the byte-exact comparison is the test suite's, against the checker).

  python tools/render3d_bench.py [--n N] [--size S] [--rounds R] [--max-steps K] [--refine B] [--out FILE]

Prints one JSON object (also written to --out).  Which unit bounds the kernel is not named here: only a separate --pmc run could.
"""
import argparse
import json
import os
import statistics
import sys

import torch                                   # torch FIRST: one HIP runtime per process
import numpy as np

sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=200 ** 3)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--max-steps", type=int, default=512)
ap.add_argument("--refine", type=int, default=8)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--out", default=None)
a = ap.parse_args()

dev = torch.device("cuda", 0)
settings, off, tick = g.dam_break_3d(a.n)
sim = g.FluidSimulation3D(settings, device=0, initial_offset=off)
sim.timed_steps(tick, a.warmup)
sim.profile(True)
sim.profile_read(True)
step_ms = sim.timed_steps(tick, a.steps) / a.steps
passes, nsteps = sim.profile_read(True)
sim.profile(False)
density_ms = passes["density"] / nsteps
p = sim.download_particles()
h = float(settings.smoothing_radius)
iso = float(np.float32(0.5) * np.float32(np.median(p["density"])))
lo, hi = p["predicted_position"].min(axis=0).astype(np.float64), p["predicted_position"].max(axis=0).astype(np.float64)
c, ext = 0.5 * (lo + hi), hi - lo
del p
S = a.size
span = 1.15 * max(ext[0], ext[1])
eye_p = c + np.float64([-0.45 * ext[0], -0.9 * ext[1], -0.5 * ext[2] - 0.9 * max(ext[0], ext[1])])
views = {"ortho": g.look_at_camera(c - [0, 0, 0.5 * ext[2] + 4 * h], c, (0, -1, 0), span, S, S, orthographic=True),
         "persp": g.look_at_camera(eye_p, c, (0, -1, 0), np.radians(50.0), S, S)}
sp = g.SurfaceParams3(iso, 0.0, 0.5 * h, a.max_steps, a.refine)
ext_stream = torch.cuda.ExternalStream(sim.stream_ptr, device=dev)
npix = S * S


def rays(cam):
    """The statement's rays as torch tensors on the device (f32)."""
    f = torch.float32
    u = ((torch.arange(cam.width, dtype=f, device=dev) + 0.5) / cam.width - 0.5)[None, :, None]
    v = ((torch.arange(cam.height, dtype=f, device=dev) + 0.5) / cam.height - 0.5)[:, None, None]
    vec = lambda q: torch.tensor([q.x, q.y, q.z], dtype=f, device=dev)      # noqa: E731
    eye, fw, ri, up = vec(cam.eye), vec(cam.forward), vec(cam.right), vec(cam.up)
    if cam.orthographic:
        o = (eye + u * ri) + v * up
        D = fw.expand_as(o)
    else:
        D = (fw + u * ri) + v * up
        o = eye.expand_as(D)
    d = D / torch.sqrt((D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2])[..., None]
    return o.reshape(-1, 3).contiguous(), d.reshape(-1, 3).contiguous()


with torch.cuda.stream(ext_stream):
    fused_out = {k: torch.zeros(npix * 10, dtype=torch.int32, device=dev) for k in views}
    rec = torch.zeros(npix * 10, dtype=torch.float32, device=dev)           # fs3_sample records of the baseline
    pts = torch.zeros((npix, 3), dtype=torch.float32, device=dev)
    ray = {k: rays(cam) for k, cam in views.items()}
torch.cuda.synchronize()


def fused(name):
    sim.render_surface(views[name], sp, out=fused_out[name].data_ptr())


def density_of(o, d, t):
    torch.addcmul(o, d, t[:, None], out=pts)
    sim.sample_device(pts.data_ptr(), npix, rec.data_ptr())
    return rec.view(npix, 10)[:, 0]


def baseline(name):
    """-> (t, steps, hit, density) of the unfused march: launches over all pixels, the mask kept by torch."""
    o, d = ray[name]
    found = torch.zeros(npix, dtype=torch.bool, device=dev)
    K = torch.full((npix,), a.max_steps, dtype=torch.int32, device=dev)
    for k in range(a.max_steps):
        t = torch.full((npix,), float(np.float32(sp.t_near) + np.float32(k) * np.float32(sp.ds)), dtype=torch.float32, device=dev)
        new = (density_of(o, d, t) >= iso) & ~found
        K = torch.where(new, torch.full_like(K, k), K)
        found |= new
    Kf = K.to(torch.float32)
    t_hi = sp.t_near + Kf * sp.ds
    t_lo = sp.t_near + (Kf - 1.0) * sp.ds
    bracket = found & (K > 0)
    for _ in range(a.refine):
        mid = 0.5 * (t_lo + t_hi)
        inside = density_of(o, d, mid) >= iso
        t_hi = torch.where(bracket & inside, mid, t_hi)
        t_lo = torch.where(bracket & ~inside, mid, t_lo)
    dens = density_of(o, d, t_hi).clone()
    hit = torch.where(found, torch.where(K > 0, 1, 2), 0)
    return torch.where(found, t_hi, torch.zeros_like(t_hi)), K, hit, dens


def window(fn, name):
    with torch.cuda.stream(ext_stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(ext_stream)
        r = fn(name)
        e1.record(ext_stream)
        e1.synchronize()
    return e0.elapsed_time(e1), r


res = {"n": a.n, "size": S, "warmup": a.warmup, "steps": a.steps, "step_ms": round(step_ms, 4), "k3_density_ms": round(density_ms, 4),
       "iso": iso, "ds": 0.5 * h, "max_steps": a.max_steps, "refine": a.refine, "rounds": a.rounds,
       "baseline_launches_per_image": a.max_steps + a.refine + 1}
for name in views:
    window(fused, name)                            # first launch of each instantiation
    _, (t, K, hit, dens) = window(baseline, name)
    got = np.frombuffer(fused_out[name].cpu().numpy().tobytes(), dtype=g.SURFACE_HIT_DTYPE)
    K, hit, t, dens = K.cpu().numpy(), hit.cpu().numpy(), t.cpu().numpy(), dens.cpu().numpy()
    agree = (got["steps"] == K) & (got["hit"] == hit)
    res[name + "_hit_fraction"] = round(float((got["hit"] != 0).mean()), 4)
    res[name + "_mean_steps"] = round(float(got["steps"].mean()), 2)
    res[name + "_pixels_agreeing_in_steps_and_hit"] = round(float(agree.mean()), 6)
    both = agree & (got["hit"] != 0)
    res[name + "_max_abs_t_difference_where_agreeing"] = float(np.abs(got["t"][both] - t[both]).max()) if both.any() else 0.0
    res[name + "_fused_ms"], res[name + "_baseline_ms"] = [], []
for r in range(a.rounds):
    order = [(fn, name) for name in views for fn in (fused, baseline)]
    for fn, name in order[r % len(order):] + order[:r % len(order)]:
        ms, _ = window(fn, name)
        res[f"{name}_{fn.__name__}_ms"].append(round(ms, 4))
for name in views:
    fm, bm = statistics.median(res[name + "_fused_ms"]), statistics.median(res[name + "_baseline_ms"])
    res[name + "_fused_median_ms"], res[name + "_baseline_median_ms"] = fm, bm
    res[name + "_fused_over_k3_density"] = round(fm / density_ms, 3)
    res[name + "_baseline_over_fused"] = round(bm / fm, 3)
sim.sync()
sim.close()
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
