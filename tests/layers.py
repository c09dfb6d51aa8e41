"""One body for the tests that every layer of the host bindings names every call of a feature: the header, the ctypes
prototypes, the library's exports, the Rust extern block and its wrapper, the C++ mirror and the Python wrapper."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-fluid-simulation_amd")
NOT_THE_WRAPPER = ("_abi.py", "build.py")      # the prototypes and the build (the glob below does not reach into multi/)


def strip_c_comments(s):
    s = re.sub(r"/\*.*?\*/", " ", s, flags=re.S)
    return re.sub(r"//[^\n]*", " ", s)


def header_text():
    return strip_c_comments(open(os.path.join(ROOT, "include", "fluidsim.h")).read())


def wrapper_text():
    """The Python wrapper: every module of the package but NOT_THE_WRAPPER."""
    paths = sorted(p for p in glob.glob(os.path.join(PKG, "*.py")) if os.path.basename(p) not in NOT_THE_WRAPPER)
    assert paths
    return "\n".join(open(p).read() for p in paths)


def assert_every_layer_names(fs, names, cls, methods):
    """Every C call of `names` is declared, prototyped, exported, bound and used by the Rust and C++ mirrors and named by the
    Python wrapper; `cls` has every method of `methods`.  The Python wrapper names a call either in full (`.fs3_xyz(`) or as
    the quoted rest of the name after the prefix of `cls` (`self._call("xyz", ...)`), and then the name must start with it."""
    header = header_text()
    rust = strip_c_comments(open(os.path.join(PKG, "rust", "src", "lib.rs")).read())
    rust_extern = re.search(r'extern\s+"C"\s*\{(.*?)\n\}', rust, flags=re.S).group(1)
    rust_rest = rust.replace(rust_extern, "")
    cpp = strip_c_comments(open(os.path.join(PKG, "host", "fluid_simulation.hpp")).read())
    py = wrapper_text()
    lib = fs.load_library()
    prefix = cls._prefix
    for name in names:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} not declared in include/fluidsim.h"
        assert name in fs._abi.PROTOTYPES, f"{name} has no ctypes prototype"
        assert hasattr(lib, name), f"{name} not exported by the library"
        assert re.search(rf"\bfn\s+{name}\s*\(", rust_extern), f"{name} not in the Rust extern block"
        assert re.search(rf"\b{name}\s*\(", rust_rest), f"{name} bound but never called by the Rust wrapper"
        assert re.search(rf"\b{name}\s*\(", cpp), f"{name} not used by the C++ mirror"
        by_stem = name.startswith(prefix) and re.search(rf"""(["']){re.escape(name[len(prefix):])}\1""", py)
        assert by_stem or re.search(rf"\.{name}\s*\(", py), f"{name} not used by the Python wrapper"
    for method in methods:
        assert hasattr(cls, method), f"{cls.__name__}.{method} missing"
    assert lib.fs_abi_version() == 2
