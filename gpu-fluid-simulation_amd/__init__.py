"""gpu-fluid-simulation_amd — MI355X-native SPH fluid-step engine (hot path of
rookieCookies/gpu-fluid-simulation) behind the C ABI in include/fluidsim.h.

This package is the thin Python host mirror used by tests and bench.py; it only
marshals arguments into libfluidsim_hip.so (hand-written HIP kernels).  There is
no CPU fallback: without the built extension (or without a GPU) calls raise.

Mirrors, by name and argument meaning:
  FluidSimulation.new / .tick / .tick_count   src/simulation.rs:139,459,12
  SimulationSettings / TickSettings           src/simulation.rs:95-122
  ResizableBuffer                             src/buffer.rs:17-88

One module per handle (sim2d, sim3d, slab, buffers) over what they share (_handle);
imaging and selftest hold the free functions, body_dynamics the host-side integrator of a dynamic 2D body.  This file only re-exports.
"""
from . import _abi
from ._abi import (  # noqa: F401
    FS_MATH_IEEE,
    FS_MATH_TOLERANCE,
    FS_MATH_WGSL_ULP,
    FS_SORT_BITONIC,
    FS_SORT_COUNTING,
    FS_SLAB_ROWMAJOR,
    FS_SLAB_SERIAL,
    FS_SLAB_STRIPS,
    MESH_VERTEX_DTYPE,
    PARTICLE3_DTYPE,
    PARTICLE_DTYPE,
    PASS_NAMES,
    SAMPLE3_DTYPE,
    SAMPLE_DTYPE,
    SURFACE_HIT_DTYPE,
    Body3Load,
    BodyLoad,
    BodyMotion,
    BodyMotion3,
    Camera3,
    ExtensionMissing,
    Nozzle,
    Nozzle3,
    Options,
    Settings,
    Settings3,
    SlabConfig,
    SurfaceParams3,
    SlabCounters,
    SortStep,
    TickSettings,
    TickSettings3,
    Uniform,
    UVec2,
    Vec2,
    Vec3,
    load_library,
)
from ._handle import FluidSimError, _check  # noqa: F401
from .body_dynamics import BodyDynamics2D, BodyDynamics3D  # noqa: F401
from .buffers import ImportedBuffer, ResizableBuffer  # noqa: F401
from .imaging import shade_surface, surface_hit_points, write_obj, write_png  # noqa: F401
from .selftest import selftest_sort, selftest_sort_policy  # noqa: F401
from .sim2d import (  # noqa: F401
    BodyLoads,
    FluidSimulation,
    SimulationSettings,
    build_uniform,
    dam_break_2d,
    default_tick_settings,
    generate_force_field,
    reference_lattice,
    rigid_motion2d,
    sort_schedule,
)
from .sim3d import BodyLoads3D, FluidSimulation3D, box_mask3d, dam_break_3d, look_at_camera, reference_lattice_3d, rigid_motion  # noqa: F401
from .slab import SlabSimulation  # noqa: F401
from .stats import Stats, Stats3D  # noqa: F401

__all__ = [
    "FluidSimulation", "ResizableBuffer", "SimulationSettings", "default_tick_settings", "dam_break_2d",
    "FluidSimError", "load_library", "PARTICLE_DTYPE", "SAMPLE_DTYPE", "SAMPLE3_DTYPE",
    "SURFACE_HIT_DTYPE", "look_at_camera", "shade_surface", "surface_hit_points", "MESH_VERTEX_DTYPE", "write_obj", "box_mask3d",
]
