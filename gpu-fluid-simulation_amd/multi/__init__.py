"""multi — multi-GPU slab driver: one process per GPU, 1-D slabs of
whole cell columns along x, one fixed-size point-to-point message per slab neighbour per
step (migrating particles + 2-column ghost halo) over RCCL (`torch.distributed`, backend
"nccl" = RCCL over xGMI).  No collective on the data path; a tiny all-reduce of the column
histogram every `rebalance_every` steps moves the slab boundaries.

The reference is single-device (src/renderer.rs:108-133): everything here is new.

Modules (so the N>1 logic is testable without GPUs):
  * `partition`  — pure numpy: the column partition, `plan_rebalance` (the boundary policy), capacities
  * `transport`  — `SlabTransport`: neighbour exchange of byte messages (host tensors on gloo, CUDA tensors on
                   nccl, the C ABI's own RCCL binding) and the re-balancing reduce that goes with each
  * `engine`     — `SlabEngine`: what the driver calls; `HipSlabEngine`, the adapter over the C ABI (`fs_slab_*`);
                   tests inject an oracle-backed engine
  * `driver`     — `SlabDriver`: the per-step protocol, generic over an engine
  * `scaling`    — the `bench.py --gpus N` entry
Importing the package imports neither torch nor the top-level bench."""
from .driver import SlabDriver, SlabProtocolError
from .engine import HipSlabEngine, SlabEngine
from .partition import (HEADER_BYTES, RECORD_BYTES, SPEED_CLAMP, boundary_columns, default_trim_margin, global_columns,
                        initial_owned, lattice_histogram, main_slots, partition_columns, plan_rebalance,
                        rebalance_boundaries, slab_capacities, travel_margin, trim_outer_edges)
from .scaling import bench_main, scaling_base
from .transport import DeviceTransport, HostTransport, NativeTransport, SlabTransport, Transport
