"""The cases tests/test_stats.py (no GPU: their conditions, on the oracle) and tests/test_stats_gpu.py (the engine against
tests/stats_ref.py) share: which hard states of tests/hard_states2d.py and tests/hard_states3d.py the after-steps tests run, the
channel values they carry, and the counts at the kernel's edges.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

f32 = np.float32

# csrc/fs_kernels.h: STATS_MAX_BLOCKS (the grid cap G), STATS_THREADS and STATS_CHUNK (particles a block takes per trip: two per
# lane).  Stated here and there; tests/test_stats.py compares the two places.
GRID_CAP, THREADS, CHUNK = 2048, 256, 512
# the kernel's edges: below, at and above a wave, a block of lanes and a chunk; then counts that depend on the cap.  G*256 + 1 and
# 2*G*256 + 77 are one and two particles per lane of a full grid: the first fills 1025 blocks with one trip each, the second makes
# block 0 take a second (ragged) trip; 2*G*512 + 3*512 + 77 makes blocks 0..2 take three full trips, the others two, and puts the
# ragged chunk in block 3's third trip.
COUNTS = [2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1025]
BIG_COUNTS = [GRID_CAP * 256 + 1, 2 * GRID_CAP * 256 + 77, 2 * GRID_CAP * CHUNK + 3 * CHUNK + 77]

# 2D: the NaN / speed-clamp / outside-the-box scene, an infinite velocity (non-finite records survive its steps), velocities of
# 2^59, the mouse impulse with an obstacle field, a corner cluster, a counting-sort configuration, two particles
CASES_2D = ["nan_clamp", "guard/inf_velocity", "guard/huge_velocities", "mouse_field", "corners/quirks/bitonic", "random/3/counting", "dam/2"]
NONFINITE_2D, DROPPED_2D = "guard/inf_velocity", "nan_clamp"            # ... after a step; nan_clamp has both in its start too
# 3D: every case of the registry runs on the GPU; these are the ones whose conditions the CPU test asserts
NONFINITE_3D, DROPPED_3D = "guard/huge_pressure", "thin/0"
STEPS = 3

SPECIALS = f32([np.nan, np.inf, -np.inf, 1e30, -1e30, 16384.0, -16384.0, np.nextafter(f32(16384.0), f32(0.0)), 0.0, -0.0, 1e-45, -1e-40,
                2.0 ** -21, -1.5 * 2.0 ** -20, 2.5 * 2.0 ** -20, 1.0, -2.5, 1000.25])


def channel_values(n, channels, seed=11):
    """[channels, n] float32: channel 0 the slot number scaled into range, channel 1 drawn from SPECIALS (NaN, infinities, values at
    and beyond 2^14, both zeros, denormals, Q ties), channel 2 uniform in (-100, 100), channel 3 left at +0.0"""
    rng = np.random.default_rng(seed + n)
    out = np.zeros((channels, n), dtype=f32)
    if channels > 0:
        out[0] = (np.arange(n, dtype=np.float64) * (1000.0 / max(n, 1))).astype(f32)
    if channels > 1:
        out[1] = SPECIALS[rng.integers(0, SPECIALS.size, size=n)]
        out[1, :min(n, SPECIALS.size)] = SPECIALS[:min(n, SPECIALS.size)]
    if channels > 2:
        out[2] = rng.uniform(-100.0, 100.0, size=n).astype(f32)
    return out


def random_records(dtype, n, seed=5):
    """n finite records in range: positions in (-50, 50), velocities in (-8, 8), densities in (0, 2000)"""
    rng = np.random.default_rng(seed + n)
    rec = np.zeros(n, dtype=dtype)
    D = rec["position"].shape[1]
    rec["position"] = rng.uniform(-50.0, 50.0, size=(n, D)).astype(f32)
    rec["predicted_position"] = rec["position"]
    rec["velocity"] = rng.uniform(-8.0, 8.0, size=(n, D)).astype(f32)
    rec["density"] = rng.uniform(0.0, 2000.0, size=n).astype(f32)
    return rec
