"""Timings of a 2D particle count that changes at run time, each mode a process of its own:
  python tools/emit2d_time.py unused <lib.so|default> [n] [warm] [steps] [sort]   the plain step, the feature never called: ms per
                                                                                  step (<lib.so>: a file in the package directory,
                                                                                  e.g. the parent commit's build; its missing
                                                                                  symbols are skipped)
  python tools/emit2d_time.py capacity [n] [warm] [steps] [rounds] [sort]         the step with capacity = count against 2 x count
  python tools/emit2d_time.py nozzle [n] [lines] [sort]                           one 4096 x 1 nozzle line: host time, call to sync
  python tools/emit2d_time.py remove [n] [share ...]                              fs_remove_in_box of about `share` of the particles:
                                                                                  host time of the blocking call, and survivors x
                                                                                  32 B over it
  python tools/emit2d_time.py after [n] [warm] [steps]                            counting mode: the steps before a one-line
                                                                                  emission against the steps after it
n defaults to 4096^2 (the dam_break_2d_16M workload of bench.py); sort is bitonic (default) or counting; times in ms."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.getcwd())
import gpu_fluid_simulation_amd as g
from gpu_fluid_simulation_amd import _abi

SURVIVOR_BYTES = 32            # position, predicted position, velocity: 8 B each; density and key: 4 B each
N16M = 4096 * 4096


def load_variant(name):
    """A build that may lack the newest symbols (the parent commit's): bind what it exports."""
    lib = C.CDLL(os.path.join("gpu-fluid-simulation_amd", name))
    for sym, (res, args) in _abi.PROTOTYPES.items():
        fn = getattr(lib, sym, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    _abi._lib = lib


def sort_of(name):
    return g.FS_SORT_COUNTING if name == "counting" else g.FS_SORT_BITONIC


def make(n, warm, capacity=0, sort="bitonic"):
    st, off, tick = g.dam_break_2d(n)
    sim = g.FluidSimulation(st, device=0, initial_offset=off, capacity=capacity, sort_mode=sort_of(sort))
    for _ in range(warm):
        sim.tick(tick)
    sim.sync()
    return sim, st, tick


def arg(k, default, kind=int):
    return kind(sys.argv[k]) if len(sys.argv) > k else default


mode = sys.argv[1] if len(sys.argv) > 1 else ""
if mode == "unused":
    variant = sys.argv[2]
    if variant != "default":
        load_variant(variant)
    n, warm, steps, sort = arg(3, N16M), arg(4, 10), arg(5, 100), arg(6, "bitonic", str)
    sim, st, tick = make(n, warm, sort=sort)
    print(f"unused {variant} {sort} n={n} steps {warm}-{warm + steps}: {sim.timed_steps(tick, steps) / steps:.4f} ms/step", flush=True)
    sim.close()
elif mode == "capacity":
    n, warm, steps, rounds, sort = arg(2, N16M), arg(3, 10), arg(4, 100), arg(5, 3), arg(6, "bitonic", str)
    out = {"capacity = count": [], "capacity = 2 x count": []}
    for _ in range(rounds):
        for name, cap in (("capacity = count", 0), ("capacity = 2 x count", 2 * n)):
            sim, st, tick = make(n, warm, cap, sort)
            out[name].append(round(sim.timed_steps(tick, steps) / steps, 4))
            sim.close()
    for name, v in out.items():
        print(f"capacity {sort} n={n} steps {warm}-{warm + steps}, {name}: {v} median {np.median(v):.4f} spread {max(v) - min(v):.4f} ms/step", flush=True)
elif mode == "nozzle":
    n, lines, sort = arg(2, N16M), arg(3, 10), arg(4, "bitonic", str)
    sim, st, tick = make(n, 10, n + 4096 * lines, sort)
    sp = st.particle_spacing
    ms = []
    for k in range(lines):
        t0 = time.perf_counter()
        sim.emit_nozzle((0.0, -0.4 * st.size.y), (sp, 0.0), (0.0, sp), (0.0, 3.0), 4096, 1)
        sim.sync()
        ms.append(round((time.perf_counter() - t0) * 1e3, 4))
        sim.tick(tick)
        sim.sync()
    print(f"nozzle {sort} n={n}: 4096 x 1 line, call to sync, host ms: {ms} median {np.median(ms):.4f} (count now {sim.particle_count})", flush=True)
    sim.close()
elif mode == "remove":
    n = arg(2, N16M)
    shares = [float(x) for x in sys.argv[3:]] or [0.01, 0.5]
    for share in shares:
        sim, st, tick = make(n, 10)
        x = sim.download_particles()["position"][:, 0]
        big = 1e6
        hi = float(np.quantile(x, share))
        sim.remove_box((big, big), (2 * big, 2 * big))                        # matches nothing: allocates the call's scratch
        t0 = time.perf_counter()
        sim.remove_box((big, big), (2 * big, 2 * big))
        print(f"remove n={n}: a box that matches nothing (flags and offsets passes, the count's read-back): "
              f"{(time.perf_counter() - t0) * 1e3:.3f} ms blocking", flush=True)
        t0 = time.perf_counter()
        removed = sim.remove_box((-big, -big), (hi, big))
        ms = (time.perf_counter() - t0) * 1e3
        left = sim.particle_count
        print(f"remove n={n}: box of about {share:.0%}: removed {removed}, {left} survivors, {ms:.3f} ms blocking; "
              f"{left * SURVIVOR_BYTES / 1e6:.1f} MB at 32 B per survivor over it: {left * SURVIVOR_BYTES / ms / 1e6:.1f} GB/s", flush=True)
        sim.tick(tick)
        sim.sync()
        sim.close()
elif mode == "after":
    n, warm, steps = arg(2, N16M), arg(3, 10), arg(4, 20)
    sim, st, tick = make(n, warm, n + 4096, "counting")
    sp = st.particle_spacing
    before = sim.timed_steps(tick, steps) / steps
    sim.emit_nozzle((0.0, -0.4 * st.size.y), (sp, 0.0), (0.0, sp), (0.0, 3.0), 4096, 1)
    first = sim.timed_steps(tick, 1)
    after = sim.timed_steps(tick, steps) / steps
    print(f"after counting n={n}: {steps} steps before the emission {before:.4f} ms/step, the first step after it {first:.4f} ms, "
          f"the {steps} steps after that {after:.4f} ms/step (count now {sim.particle_count})", flush=True)
    sim.close()
else:
    raise SystemExit(__doc__)
