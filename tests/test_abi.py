"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol
include/fluidsim.h declares, and its pure host mirrors (lattice, sort schedule, uniform)
agree with the oracle bit for bit.  No compute calls (no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    text = open(os.path.join(ROOT, "include", "fluidsim.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fs3?_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(fs):
    lib = fs.load_library()
    names = _declared_symbols()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/fluidsim.h but not exported"
    assert set(names) == set(fs._abi.PROTOTYPES), "ctypes prototypes out of sync with the header"
    assert lib.fs_abi_version() == 2


def test_struct_sizes_match_header(fs):
    assert C.sizeof(fs.Settings) == 28 and C.sizeof(fs.TickSettings) == 60
    assert C.sizeof(fs.Uniform) == 120 and C.sizeof(fs.Options) == 32 and C.sizeof(fs.SortStep) == 16


@pytest.mark.parametrize("n", [2, 3, 4096, 5000, 100_000, 1 << 20])
def test_sort_schedule_matches_oracle(fs, orc, n):
    got = fs.sort_schedule(n)
    cnt = orc.lib().orc_sort_schedule(n, None, 0)
    arr = (fs.SortStep * cnt)()
    orc.lib().orc_sort_schedule(n, arr, cnt)
    assert got == [(a.group_width, a.group_height, a.step_index, a.num_values) for a in arr]


@pytest.mark.parametrize("n,off", [(4096, (0.0, 0.0)), (100_000, (0.0, 0.0)), (1 << 20, (-51.15, 12.75)), (7, (1.0, 2.0))])
def test_reference_lattice_matches_oracle(fs, orc, n, off):
    st = fs.SimulationSettings(n, 0.1, 0.2, (53, 53))
    got = fs.reference_lattice(st, off)
    want = np.zeros(n, dtype=fs.PARTICLE_DTYPE)
    orc.lib().orc_lattice(C.addressof(st), off[0], off[1], want.ctypes.data, n)
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8))


def test_build_uniform_matches_oracle(fs, orc):
    st = fs.SimulationSettings(12345, 0.1, 0.23, (17.0, 9.5), (512, 256))
    t = fs.default_tick_settings(gravity=(0.3, 9.81), mouse_state=-1, mouse_pos=(1.0, -2.0))
    got = fs.build_uniform(st, t, 41)
    want = fs.Uniform()
    orc.lib().orc_build_uniform(C.addressof(st), C.addressof(t), 41, C.addressof(want))
    assert bytes(got) == bytes(want)


def test_invalid_settings_rejected_without_device(fs):
    # N <= 1 panics in the reference (ilog2(0), simulation.rs:323-324) -> FS_ERR_INVALID here
    for n in (0, 1):
        with pytest.raises(fs.FluidSimError) as e:
            fs.FluidSimulation(fs.SimulationSettings(n, 0.1, 0.2, (53, 53)))
        assert e.value.status == fs._abi.FS_ERR_INVALID
    with pytest.raises(fs.FluidSimError) as e:
        fs.FluidSimulation(fs.SimulationSettings(100, 0.1, 0.0, (53, 53)))
    assert e.value.status == fs._abi.FS_ERR_INVALID


def _hip_device_count(fs):
    """Devices seen by the HIP runtime the engine library is linked against.  torch is no witness here: imported after
    that runtime is loaded (the fs fixture loads it first), torch.cuda.is_available() can be False on a machine with a GPU."""
    fs.load_library()
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
    n = C.c_int(0)
    return n.value if C.CDLL(path).hipGetDeviceCount(C.byref(n)) == 0 else 0


def test_no_cpu_fallback(fs):
    """Without a GPU the engine must fail loudly, never compute on the host."""
    if _hip_device_count(fs) > 0:
        pytest.skip("GPU present")
    with pytest.raises(fs.FluidSimError) as e:
        fs.FluidSimulation(fs.SimulationSettings(4096, 0.1, 0.2, (53, 53)))
    assert e.value.status == fs._abi.FS_ERR_DEVICE


def test_missing_extension_fails_loudly(fs, tmp_path):
    with pytest.raises(fs.ExtensionMissing):
        fs.load_library(str(tmp_path / "nope.so"))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "gpu-fluid-simulation_amd")
    for dp, _, files in os.walk(pkg):
        if os.path.basename(dp) == "build":
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", ".hpp", ".rs")):
                src = open(os.path.join(dp, f), errors="replace").read()
                # no include / import / dlopen of anything under oracle/ (comments may cite it)
                assert not re.search(r'#\s*include\s*[<"][^>"]*oracle', src), f
                assert not re.search(r'^\s*(from|import)\s+oracle', src, flags=re.M), f
                assert "libsph_oracle" not in src, f


def test_header_is_plain_c(fs, tmp_path):
    """include/fluidsim.h must be usable from C (the FFI boundary): compile and link a C99 program
    that references every declared entry point and checks the POD sizes."""
    import subprocess
    names = _declared_symbols()
    lines = ['#include "include/fluidsim.h"', "#include <stdio.h>", "typedef void (*fn_t)(void);",
             "static const fn_t table[] = {"]
    lines += [f"    (fn_t){n}," for n in names]
    lines += ["};", "int main(void) {",
              "    if (sizeof(fs_particle) != 32 || sizeof(fs_uniform) != 120 || sizeof(fs_settings) != 28) return 2;",
              "    if (sizeof(fs_tick_settings) != 60 || sizeof(fs3_particle) != 48 || sizeof(fs_options) != 32) return 3;",
              '    printf("abi %d symbols %d\n", fs_abi_version(), (int)(sizeof table / sizeof table[0]));'.replace("\n", "\\n"),
              "    return 0;", "}"]
    src = tmp_path / "abi_c99.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "abi_c99"
    libdir = os.path.join(ROOT, "gpu-fluid-simulation_amd")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", ROOT, str(src), "-o", str(exe), "-L", libdir,
                           "-lfluidsim_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert f"abi 2 symbols {len(names)}" in out.stdout


def test_comm_failure_is_fs_err_comm(fs, tmp_path):
    """RCCL problems surface as FS_ERR_COMM through the ABI (never an abort): here librccl itself cannot be loaded."""
    import subprocess, sys
    code = ("import sys, ctypes as C; sys.path.insert(0, %r); import gpu_fluid_simulation_amd as g; lib = g.load_library(); "
            "b = (C.c_uint8 * 128)(); rc = lib.fs_comm_unique_id(b); print(rc, lib.fs_last_error().decode())" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, FS_RCCL_LIB=str(tmp_path / "no_such_librccl.so")))
    assert out.returncode == 0, out.stderr
    assert out.stdout.startswith("5 "), out.stdout          # FS_ERR_COMM
    assert "librccl" in out.stdout


def test_build_recipe_lists_every_included_header():
    """a header the sources include but build.py does not list neither rebuilds the objects nor trips is_stale()
    (bench.py --no-build would accept a stale library).  Every quoted #include under csrc/ must be a listed header."""
    import importlib.util
    import re
    spec = importlib.util.spec_from_file_location("fs_build", os.path.join(ROOT, "gpu-fluid-simulation_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    listed = {os.path.normpath(os.path.join(b.CSRC, h)) for h in b.HEADERS}
    seen = set()
    for name in sorted(os.listdir(b.CSRC)):
        if not name.endswith((".hip", ".h", ".hpp")):
            continue
        for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(os.path.join(b.CSRC, name)).read(), flags=re.M):
            seen.add(os.path.normpath(os.path.join(b.CSRC, inc)))
    assert seen, "no quoted includes found: the scan is broken"
    missing = sorted(p for p in seen if p not in listed)
    assert not missing, f"included under csrc/ but not in build.py HEADERS: {missing}"
    assert all(os.path.exists(p) for p in listed), "build.py lists a header that does not exist"
    assert set(os.listdir(b.CSRC)) >= set(b.SOURCES), "build.py lists a source that does not exist"
    # and the other way round: a csrc/*.hip that is not built, or a csrc/*.h whose edits trigger no rebuild
    on_disk = sorted(os.listdir(b.CSRC))
    unbuilt = [n for n in on_disk if n.endswith(".hip") and n not in b.SOURCES]
    assert not unbuilt, f"under csrc/ but not in build.py SOURCES: {unbuilt}"
    unlisted = [n for n in on_disk if n.endswith(".h") and n not in b.HEADERS]
    assert not unlisted, f"under csrc/ but not in build.py HEADERS: {unlisted}"
