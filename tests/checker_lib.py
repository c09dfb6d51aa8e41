"""The one place that builds and loads a checker: a translation unit under tests/ that includes the oracle's sources unchanged
and adds the statement of one feature (tests/*_checker.cpp, loaded by the tests/*_ref.py modules).  TEST INFRASTRUCTURE ONLY.

build() compiles with the oracle's own code-generation flags (oracle/oracle.py FLAGS, held to oracle/Makefile by
tests/test_support.py) into a per-user cache directory outside the tree (the checkout may be read-only).  The file name carries
a hash of every source and of the flags, so an edit yields a new file and an old one is never loaded for new sources.
load() opens the library once per stem and gives it the oracle's prototypes."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ORACLE_2D = [os.path.join(ROOT, "oracle", "sph_oracle.cpp"), os.path.join(ROOT, "include", "fluidsim.h")]
ORACLE_3D = [os.path.join(ROOT, "oracle", "sph_oracle3d.cpp"), os.path.join(ROOT, "include", "fluidsim.h")]
FLAGS = O.FLAGS + ["-shared"]

_libs = {}


def here(name):
    return os.path.join(HERE, name)


def cache_dir():
    d = os.path.join(tempfile.gettempdir(), f"fs_checkers_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    return d


def path_of(stem, sources):
    """-> where the library of these sources lives: lib<stem>_<hash of every source's contents and of the flags>.so"""
    h = hashlib.sha256()
    for s in sources:
        with open(s, "rb") as f:
            h.update(f.read())
    h.update(" ".join(FLAGS).encode())
    return os.path.join(cache_dir(), f"lib{stem}_{h.hexdigest()[:16]}.so")


def build(stem, sources):
    """-> path_of(stem, sources), compiled if it is not there yet.  sources[0] is the translation unit; the others are what it
    includes.  Compiled to a name of this process's own and installed with os.replace, so concurrent pytest workers never load
    half a file."""
    out = path_of(stem, sources)
    if not os.path.exists(out):
        tmp = f"{out}.{os.getpid()}.tmp"
        subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + ["-o", tmp, sources[0]])
        os.replace(tmp, out)
    return out


def load(stem, sources, family, own):
    """-> the checker's library, opened once per stem, with the argtypes and restype of every oracle entry point of `family`
    ("orc_": the 2D oracle's, "orc3_": the 3D oracle's; neither prefix matches the other's names) that oracle.lib() declares,
    and those of the checker's own entry points: own = {name: (restype, argtypes)}."""
    assert family in ("orc_", "orc3_")
    if stem not in _libs:
        L = C.CDLL(build(stem, sources))
        for name, f in list(O.lib().__dict__.items()):
            if name.startswith(family):
                g = getattr(L, name)
                g.argtypes, g.restype = f.argtypes, f.restype
        for name, (restype, argtypes) in own.items():
            g = getattr(L, name)
            g.argtypes, g.restype = argtypes, restype
        if family == "orc_":
            L.orc_set_threads(1)                    # as oracle.lib(): a scalar port unless a caller asks for more
        _libs[stem] = L
    return _libs[stem]
