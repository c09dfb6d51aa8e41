"""Build recipe: hipcc --offload-arch=gfx950 -> gpu-fluid-simulation_amd/libfluidsim_hip.so (in-tree).

-ffp-contract=off keeps the kernels' f32 arithmetic in the written association
(no FMA contraction) so results match the CPU oracle bit for bit.
-fno-slp-vectorize (float kernels, see NO_SLP): at -O3 the SLP vectoriser packs adjacent scalar f32 mul/add into v_pk_* ops;
on gfx950 those issue at half rate and cost extra v_mov to line the operands up (measured at 16M:
force 0.93 -> 0.85 ms, density 0.30 -> 0.29 ms without it; same bits either way).

SOURCES are the translation units; HEADERS is everything else a unit reads — the headers and the .inc fragments that are
compiled as part of kernels_sort.hip and kernels_force.hip — so that touching any of them makes the library stale.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libfluidsim_hip.so")
SOURCES = ["engine.hip", "engine_features.hip", "engine_query.hip", "engine_count.hip", "engine_selftest.hip", "engine_slab.hip", "comm.hip", "buffer.hip", "kernels_reorder.hip", "kernels_density.hip", "kernels_render.hip", "kernels_force.hip", "kernels_proof.hip", "kernels_sort.hip", "kernels_slab.hip", "kernels_strip.hip", "kernels_csort.hip", "kernels_field.hip", "kernels_track.hip", "kernels_diffuse.hip", "kernels_sample.hip", "kernels_count.hip", "kernels_bodies.hip", "kernels_3d.hip", "kernels_density3d.hip", "kernels_force3d.hip", "kernels_sample3d.hip", "kernels_sample_attr3d.hip", "kernels_render3d.hip", "kernels_mesh3d.hip", "kernels_collide3d.hip", "kernels_bodies3d.hip", "kernels_diffuse3d.hip", "kernels_stats.hip", "kernels_stats3d.hip", "engine_stats.hip", "engine_3d.hip", "engine_3d_features.hip", "engine_3d_query.hip", "engine_3d_count.hip", "engine_3d_stats.hip"]
HEADERS = ["engine.h", "engine_3d.h", "engine_bodies.h", "engine_count.h", "fs_3d.h", "fs_body_loads.h", "fs_count.h", "fs_csort_layout.h", "fs_device.h", "fs_field3.h", "fs_force_lists.h", "fs_force_pair.h", "fs_force_sweep.h", "fs_host.h", "fs_kernels.h", "fs_neighbours.h", "fs_sample3.h", "fs_scan.h", "fs_slab.h", "fs_sort.h", "fs_sort_tile.h", "fs_stats.h", "fs_sweep3.h", "kernels_force_quad.inc", "kernels_sort_tile.inc", "kernels_sort_global.inc", "sort_policy.h", os.path.join("..", "..", "include", "fluidsim.h")]
FLAGS = [
    "--offload-arch=gfx950",
    "-O3",
    "-std=c++17",
    "-fPIC",
    "-ffp-contract=off",
    "-fno-fast-math",
    "-Wall",
    "-Wno-unused-function",
]


# kernels_sort_tile.inc and kernels_sort_global.inc are compiled as part of kernels_sort.hip (see its last lines): HEADERS.
# kernels_force_quad.inc likewise, as part of kernels_force.hip (it uses that file's integrator and parameter list).
# float-heavy kernels only: the integer sort kernels measured ~1 % faster with the vectoriser on
# (kernels_reorder.hip and kernels_proof.hip hold no such arithmetic; the flag is the one their kernels were measured with)
NO_SLP = {"kernels_reorder.hip", "kernels_density.hip", "kernels_render.hip", "kernels_force.hip", "kernels_proof.hip", "kernels_3d.hip", "kernels_density3d.hip", "kernels_force3d.hip", "kernels_slab.hip", "kernels_strip.hip", "kernels_sample.hip", "kernels_sample3d.hip", "kernels_sample_attr3d.hip", "kernels_render3d.hip", "kernels_mesh3d.hip", "kernels_bodies3d.hip", "kernels_bodies.hip", "kernels_diffuse.hip", "kernels_diffuse3d.hip", "kernels_stats.hip", "kernels_stats3d.hip"}


def _flags(src):
    return FLAGS + (["-fno-slp-vectorize"] if os.path.basename(src) in NO_SLP else [])


def _stale(out, deps):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def is_stale():
    """True when the library is missing or older than any source/header (what build() would act on)."""
    deps = [os.path.join(CSRC, s) for s in SOURCES] + [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]
    return _stale(OUT, deps)


def build(force=False, verbose=True, out=None, extra_flags=()):
    """Compile and link.  `out`/`extra_flags` build an experimental variant next to the default library."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if out is not None:
        return _build_variant(hipcc, out, list(extra_flags), verbose)
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.abspath(__file__)]
    objs = []
    procs = []
    for src in SOURCES:
        sp = os.path.join(CSRC, src)
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        objs.append(obj)
        if force or _stale(obj, [sp] + hdrs):
            cmd = [hipcc] + _flags(sp) + ["-c", sp, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((src, subprocess.Popen(cmd)))
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {src}")
    if force or procs or _stale(OUT, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs + ["-ldl"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return OUT


def _build_variant(hipcc, out, extra, verbose):
    """Same per-source flags as the default build plus `extra`; objects go to build/<variant>/."""
    objdir = os.path.join(HERE, "build", os.path.splitext(os.path.basename(out))[0])
    os.makedirs(objdir, exist_ok=True)
    procs, objs = [], []
    for src in SOURCES:
        sp = os.path.join(CSRC, src)
        obj = os.path.join(objdir, src.replace(".hip", ".o"))
        objs.append(obj)
        cmd = [hipcc] + _flags(sp) + extra + ["-c", sp, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((src, subprocess.Popen(cmd)))
    for src, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {src}")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs + ["-ldl"])
    return out


if __name__ == "__main__":
    build(force="--force" in sys.argv)
