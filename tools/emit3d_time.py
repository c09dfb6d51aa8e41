"""Timings of a 3D particle count that changes at run time, each mode a process of its own:
  python tools/emit3d_time.py unused <lib.so|default> [n] [warm] [steps]   the plain step, the feature never called: ms per step
                                                                           (<lib.so>: a file in the package directory, e.g. the
                                                                           parent commit's build; its missing symbols are skipped)
  python tools/emit3d_time.py capacity [n] [warm] [steps] [rounds]         the step with capacity = count against capacity = 2 x count
  python tools/emit3d_time.py nozzle [n] [layers]                          one 64 x 64 nozzle layer: host time, call to sync
  python tools/emit3d_time.py remove [n] [share ...]                       fs3_remove_in_box of about `share` of the particles: host
                                                                           time of the blocking call, and survivors x 52 B over it
n defaults to 200^3 (the dam_break_3d_8M workload of bench.py); times in ms."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g
from gpu_fluid_simulation_amd import _abi

SURVIVOR_BYTES = 52            # position, velocity, predicted position + density: 16 B each; the key: 4 B


def load_variant(name):
    """A build that may lack the newest symbols (the parent commit's): bind what it exports."""
    lib = C.CDLL(os.path.join("gpu-fluid-simulation_amd", name))
    for sym, (res, args) in _abi.PROTOTYPES.items():
        fn = getattr(lib, sym, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    _abi._lib = lib


def make(n, warm, capacity=None):
    st, off, tick = g.dam_break_3d(n)
    sim = g.FluidSimulation3D(st, device=0, initial_offset=off)
    if capacity:
        sim.reserve(capacity)
    for _ in range(warm):
        sim.tick(tick)
    sim.sync()
    return sim, st, tick


def arg(k, default, kind=int):
    return kind(sys.argv[k]) if len(sys.argv) > k else default


mode = sys.argv[1]
if mode == "unused":
    variant = sys.argv[2]
    if variant != "default":
        load_variant(variant)
    n, warm, steps = arg(3, 200 ** 3), arg(4, 10), arg(5, 100)
    sim, st, tick = make(n, warm)
    print(f"unused {variant} n={n} steps {warm}-{warm + steps}: {sim.timed_steps(tick, steps) / steps:.4f} ms/step", flush=True)
    sim.close()
elif mode == "capacity":
    n, warm, steps, rounds = arg(2, 200 ** 3), arg(3, 10), arg(4, 100), arg(5, 3)
    out = {"capacity = count": [], "capacity = 2 x count": []}
    for _ in range(rounds):
        for name, cap in (("capacity = count", None), ("capacity = 2 x count", 2 * n)):
            sim, st, tick = make(n, warm, cap)
            out[name].append(round(sim.timed_steps(tick, steps) / steps, 4))
            sim.close()
    for name, v in out.items():
        print(f"capacity n={n} steps {warm}-{warm + steps}, {name}: {v} median {np.median(v):.4f} spread {max(v) - min(v):.4f} ms/step", flush=True)
elif mode == "nozzle":
    n, layers = arg(2, 200 ** 3), arg(3, 10)
    sim, st, tick = make(n, 10, n + 4096 * layers)
    sp = st.particle_spacing
    ms = []
    for k in range(layers):
        t0 = time.perf_counter()
        sim.emit_nozzle((0.0, -0.4 * st.size.y, 0.0), (sp, 0.0, 0.0), (0.0, 0.0, sp), (0.0, 3.0, 0.0), 64, 64)
        sim.sync()
        ms.append(round((time.perf_counter() - t0) * 1e3, 4))
        sim.tick(tick)
        sim.sync()
    print(f"nozzle n={n}: 64 x 64 layer, call to sync, host ms: {ms} median {np.median(ms):.4f} (count now {sim.particle_count})", flush=True)
    sim.close()
elif mode == "remove":
    n = arg(2, 200 ** 3)
    shares = [float(x) for x in sys.argv[3:]] or [0.01, 0.5]
    for share in shares:
        sim, st, tick = make(n, 10)
        x = sim.download_particles()["position"][:, 0]
        big = 1e6
        hi = float(np.quantile(x, share))
        sim.remove_box((big, big, big), (2 * big, 2 * big, 2 * big))          # matches nothing: allocates the call's scratch
        t0 = time.perf_counter()
        sim.remove_box((big, big, big), (2 * big, 2 * big, 2 * big))
        print(f"remove n={n}: a box that matches nothing (flags and offsets passes, the count's read-back): "
              f"{(time.perf_counter() - t0) * 1e3:.3f} ms blocking", flush=True)
        t0 = time.perf_counter()
        removed = sim.remove_box((-big, -big, -big), (hi, big, big))
        ms = (time.perf_counter() - t0) * 1e3
        left = sim.particle_count
        print(f"remove n={n}: box of about {share:.0%}: removed {removed}, {left} survivors, {ms:.3f} ms blocking; "
              f"{left * SURVIVOR_BYTES / 1e6:.1f} MB at 52 B per survivor over it: {left * SURVIVOR_BYTES / ms / 1e6:.1f} GB/s", flush=True)
        sim.tick(tick)
        sim.sync()
        sim.close()
else:
    raise SystemExit(__doc__)
