"""The cost of the fluid diagnostics, to be run on the GPU:
  python tools/stats_time.py [warm_steps] [calls] [reps] [cases]
For the 16 M particle 2D and the 8 M particle 3D bench scenes (cases: 2d, 3d or both), with 0 and 4 tracking channels, after
`warm_steps` steps: the time of one fs_stats_device / fs3_stats_device call (k_stats + k_stats_fold), taken over `calls`
back-to-back calls between two events on the handle's stream; the bytes per second that implies for the bytes the kernel reads
(2D after a step: 24 B per particle — positions, velocities and the {rho, 1/rho} pairs — plus 4 B per channel; 3D: 48 B plus 4 B
per channel); and, for scale, the time of a device-to-device copy that READS the same number of bytes (and writes as many), taken
the same way in the same process.  One line per case and repetition."""
import os, sys
sys.path.insert(0, os.getcwd())
import torch                                   # torch first: one HIP runtime per process
import numpy as np
import gpu_fluid_simulation_amd as g
warm = int(sys.argv[1]) if len(sys.argv) > 1 else 10
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 200
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
cases = {"2d": ["2d"], "3d": ["3d"], "both": ["2d", "3d"]}[sys.argv[4] if len(sys.argv) > 4 else "both"]
dev = torch.device("cuda", 0)


def timed(stream, fn, count):
    """ms per call of `fn`, `count` calls between two events on `stream`"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(stream)
    for _ in range(count):
        fn()
    t1.record(stream)
    t1.synchronize()
    return t0.elapsed_time(t1) / count


for rep in range(reps):
    for case in cases:
        for channels in (0, 4):
            if case == "2d":
                st, off, tick = g.dam_break_2d(4096 ** 2)
                sim = g.FluidSimulation(st, device=0, initial_offset=off, track=channels if channels else None)
                per_particle, size = 24 + 4 * channels, 208
            else:
                st, off, tick = g.dam_break_3d(200 ** 3)
                sim = g.FluidSimulation3D(st, device=0, initial_offset=off, track=channels if channels else None)
                per_particle, size = 48 + 4 * channels, 232
            n = sim.particle_count
            for c in range(channels):
                sim.set_attribute(c, np.linspace(-50.0, 50.0, n).astype(np.float32))
            for _ in range(warm):
                sim.tick(tick)
            sim.sync()
            ext = torch.cuda.ExternalStream(sim.stream_ptr, device=dev)
            nbytes = n * per_particle
            with torch.cuda.stream(ext):
                out = torch.zeros(size // 8, dtype=torch.int64, device=dev)
                src = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
                dst = torch.empty_like(src)
                torch.cuda.synchronize()
                stats = lambda: sim.stats_device_ptr(out.data_ptr())
                copy = lambda: dst.copy_(src)
                for _ in range(5):
                    stats(); copy()
                ms_stats = timed(ext, stats, calls)
                ms_copy = timed(ext, copy, calls)
            s = sim.stats()
            assert s.to_bytes() == out.cpu().numpy().tobytes() and s.count == n
            print(f"stats {case} n={n} channels {channels} rep {rep}: {ms_stats * 1e3:.1f} us/call, {nbytes / ms_stats / 1e9:.3f} TB/s over "
                  f"{per_particle} B/particle; d2d copy reading the same bytes {ms_copy * 1e3:.1f} us ({nbytes / ms_copy / 1e9:.3f} TB/s read); "
                  f"ratio {ms_stats / ms_copy:.2f}; nonfinite {s.nonfinite} dropped {s.dropped} max speed {s.max_speed():.3f}", flush=True)
            del src, dst, out
            sim.close()
