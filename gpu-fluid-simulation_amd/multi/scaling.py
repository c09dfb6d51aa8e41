"""bench.py --gpus N (N > 1): the strong-scaling run over N slabs, and its one-rank base."""
import json
import os
import time

import numpy as np

from .driver import SlabDriver
from .engine import HipSlabEngine
from .partition import (HEADER_BYTES, RECORD_BYTES, default_trim_margin, initial_owned, lattice_histogram, main_slots,
                        partition_columns, slab_capacities, trim_outer_edges)
from .transport import NativeTransport, Transport


def scaling_base(g, settings, off, tick, gh, gw, device_index, warmup, steps):
    """ms/step of the slab engine as ONE rank over the whole domain (no neighbours, no exchange), same window."""
    n = settings.particle_count
    cap, recv = slab_capacities(n, 1, gh)
    sim = g.SlabSimulation(settings, 0, gw, False, False, cap, recv, gw, device=device_index)
    sim.upload_owned(g.reference_lattice(settings, off))
    for _ in range(warmup):
        sim.pack(tick, None, None); sim.step(None, None)
    sim.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        sim.pack(tick, None, None); sim.step(None, None)
    sim.sync()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    ok = sim.counters()
    sim.close()
    return {"ms_per_step": round(ms, 4), "value": round(n / (ms * 1e-3) / 1e6, 2), "unit": "M particle-steps/s",
            "n_gpus": 1, "engine": "slab engine, 1 rank, counting sort", "violations": ok["lost"] + ok["overflow"] + ok["far_halo"]}


def bench_main(args, rank, local_rank, world):
    """bench.py --gpus N (N > 1): strong scaling of the 16M dam break over N slabs."""
    import torch
    import torch.distributed as dist
    import gpu_fluid_simulation_amd as g
    from bench import ALG_BYTES, ALG_TOTAL, HBM_COPY_GBS, HBM_PEAK_GBS, WORKLOADS, bound_from_evidence, load_json

    backend = os.environ.get("FS_DIST_BACKEND", "nccl")
    if os.environ.get("FS_FORCE_DEVICE0"):      # single-GPU rehearsal: every rank on device 0 (gloo only)
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dist.init_process_group(backend=backend, rank=rank, world_size=world,
                            device_id=torch.device("cuda", local_rank) if backend == "nccl" else None)
    n = WORKLOADS[args.workload]
    settings, off, tick = g.dam_break_2d(n)
    hist, gw = lattice_histogram(g, settings, off)
    gh = int(np.ceil(np.float32(settings.size.y) / np.float32(settings.smoothing_radius))) + 2
    bounds = partition_columns(hist, world)
    cap, recv = slab_capacities(n, world, gh)
    max_cols = gw      # tables for the whole grid (42 MB each at 16M): the outer-edge margin follows the fluid's speed
    rebalance_every = int(os.environ.get("FS_REBALANCE_EVERY", "64"))
    # outer slabs: occupied columns + margin — only while re-balancing keeps moving the edges with the fluid
    bounds = trim_outer_edges(bounds, hist, default_trim_margin() if rebalance_every > 0 else 0)
    msg_bytes = HEADER_BYTES + RECORD_BYTES * recv
    dev = torch.device("cuda", local_rank) if backend == "nccl" else None
    native = bool(os.environ.get("FS_NATIVE_RCCL")) and backend == "nccl"
    if native:      # the C ABI's own RCCL binding (fs_slab_exchange): what a non-Python host would run
        tr = NativeTransport(g, rank, world, msg_bytes, local_rank, dist, reduce_device=dev)
    else:
        tr = Transport(rank, world, msg_bytes, device=dev)
    eng = HipSlabEngine(g, settings, bounds, rank, world, cap, recv, max_cols, local_rank, tr)
    assert eng.message_bytes == msg_bytes
    eng.sim.upload_owned(initial_owned(g, settings, off, bounds, rank))
    drv = SlabDriver(eng, tr, bounds, gw, rebalance_every=rebalance_every, capacity_main=main_slots(cap, recv), max_cols=max_cols)

    ext = torch.cuda.ExternalStream(eng.sim.stream_ptr, device=torch.device("cuda", local_rank))
    with torch.cuda.stream(ext):
        for _ in range(args.warmup):
            drv.step(tick)
        eng.sync()
        torch.cuda.synchronize()
        dist.barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            drv.step(tick)
        eng.sync()
        torch.cuda.synchronize()
        dist.barrier()
        elapsed = time.perf_counter() - t0
        # after the timed region: a short window with a HIP event at every pass boundary of THIS rank's stream (all ranks
        # keep stepping in lockstep), for the roofline of the dominant pass
        eng.sim.profile(True)
        eng.sim.profile_read(reset=True)
        prof_steps = max(1, min(args.steps, 20))
        for _ in range(prof_steps):
            drv.step(tick)
        eng.sync()
        passes, psteps = eng.sim.profile_read(reset=True)
        eng.sim.profile(False)
    on = dev if dev is not None else "cpu"
    tmax = torch.tensor([elapsed], dtype=torch.float64, device=on)
    dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    cnt = eng.counters()
    bad = torch.tensor([cnt["lost"] + cnt["overflow"] + cnt["far_halo"]], dtype=torch.int64, device=on)
    dist.all_reduce(bad)
    nlive = torch.tensor([int(eng.owned_particles().shape[0])], dtype=torch.int64, device=on)
    dist.all_reduce(nlive)
    base = None
    if rank == 0 and not os.environ.get("FS_NO_SCALING_BASE"):
        base = scaling_base(g, settings, off, tick, gh, gw, local_rank, args.warmup, args.steps)
    if rank == 0:
        ms_per_step = float(tmax.item()) * 1e3 / args.steps
        value = n / (ms_per_step * 1e-3) / 1e6
        agg = ALG_TOTAL * n / (ms_per_step * 1e-3) / 1e9
        # dominant pass of rank 0 (its share of the particles): algorithmic bytes / its measured time; the bound comes
        # from the committed counter summary of that pass's kernel, as for N = 1 — never assumed
        n_rank = int(cnt["n_live"])
        alg = dict(ALG_BYTES, predict_key=28, sort=12)           # slabs: pack (predict + key + messages) is its own pass
        pp = {k: v / max(psteps, 1) for k, v in passes.items() if k in alg}
        # the `predict_key` interval of a slab step is pack + the halo exchange + unpack: communication, not a kernel —
        # it is reported beside the roofline (pack_exchange_ms); the roofline's kernel is the longest COMPUTE pass
        kernels_only = {k: v for k, v in pp.items() if k != "predict_key"} or pp
        dom = max(kernels_only, key=kernels_only.get)
        dom_gbs = alg[dom] * n_rank / (pp[dom] * 1e-3) / 1e9 if pp[dom] > 0 else 0.0
        bound, crow = bound_from_evidence(dom, dom_gbs / HBM_COPY_GBS, load_json("counters_latest.json"), False)
        out = {
            "metric": "M particle-steps/s", "value": round(value, 2), "unit": "M particle-steps/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": args.workload, "particles": n, "scene": "SURVEY.md §8d dam_break_2d",
                       "sort": "counting (slab default: per-rank sorts are tolerance-parity by construction)",
                       "parallelism": f"{world} column slabs, RCCL p2p halo ({backend}" + (", C-ABI fs_slab_exchange)" if native else ", torch.distributed)"),
                       "slab_columns": [drv.bounds[k + 1] - drv.bounds[k] for k in range(world)],
                       "outer_trim_margin": drv.trim_margin,
                       "message_bytes": msg_bytes},
            "roofline": {"bound": bound, "kernel": f"{dom} pass of rank 0 ({n_rank} live particles incl. ghosts)",
                         "achieved": round(dom_gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(dom_gbs / HBM_PEAK_GBS, 4), "traffic": None,
                         "valu_issue_frac_of_kernel": crow.get("valu_issue_frac") if crow else None,
                         "rank0_passes_ms": {k: round(v, 4) for k, v in pp.items()},
                         "pack_exchange_ms": round(pp.get("predict_key", 0.0), 4),
                         "exchange_longer_than_kernel": bool(pp.get("predict_key", 0.0) > pp[dom]),
                         "step_aggregate": {"alg_bytes_per_particle": ALG_TOTAL, "achieved": round(agg, 1),
                                            "peak": HBM_PEAK_GBS * world, "frac": round(agg / (HBM_PEAK_GBS * world), 4)}},
            "checks": {"particles_conserved": int(nlive.item()) == n, "protocol_violations": int(bad.item())},
            "slab_step": {0: "serial (pack -> exchange -> step)", 1: "edge-first (next step's messages built and exchanged beside the interior "
                          "columns' force pass; column-major cell ids on ranks with neighbours)", 2: "strips (interior while the messages "
                          "fly, boundary strips afterwards)"}[eng.sim.step_mode],
            "boundary_cols": drv.last_boundary,
            # like-for-like base of the scaling curve: N = 1 of bench.py runs the PLAIN engine with the reference
            # network; this is the SAME slab engine (counting sort, fixed-capacity slots, pack/unpack) as ONE rank
            "scaling_base": base,
            "multi_gpu_note": "8-GPU timing is produced by the driver's SCALE run only; this builder's boxes have one GPU",
        }
        if not args.no_cpu_baseline:     # rank 0, after the timed region (the other ranks wait in the barrier below)
            from bench import cpu_baseline
            out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out), flush=True)
    dist.barrier()
    dist.destroy_process_group()
