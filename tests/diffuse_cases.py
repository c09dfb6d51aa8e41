"""The cases of the diffusion / buoyancy tests, shared by tests/test_diffusion.py (the checker alone: the cases
test what they say) and tests/test_diffusion_gpu.py (the engine against the checker).  TEST INFRASTRUCTURE ONLY: plain numpy on
tests/diffuse_ref.DiffuseChecker, no GPU.

A registry run takes a case of tests/hard_states2d.py in one sort mode with four channels:
    0  finite values of both signs up to 1e30 (hard_states2d.sample_channel_values), diffusing, and the buoyancy channel
    1  negative zeros, kappa = 0: must come back as a bit copy of what tracking alone gives
    2  finite values, diffusing four times as fast (g R up to 2: past the stable range, still bit for bit)
    3  NaN payloads, +-inf, -0.0 and denormals (bitcmp.special_bits, the twelve-value pool at seed 99), diffusing
kappa is chosen from the checker's R of the first step so that g R = 1/2 where R is largest among the finite ones."""
import functools

import numpy as np

from tests import bitcmp
from tests import hard_states2d as H

f32 = np.float32
SORTS = ("bitonic", "counting")
NB_TILE = 640                      # fs_neighbours.h: a block whose row range is longer takes the unstaged sweep
CHANNELS = 4
BETA, REFERENCE = 0.01, 0.0


special_bits = functools.partial(bitcmp.special_bits, seed=99, pool=bitcmp.POOL_TWELVE)      # special_bits(n), as the tracking tests draw it


def kappa_for(R, delta, target):
    """the conductivity at which g R = (2 kappa delta) R is `target` where R is largest among the finite, positive values; 1 when
    there is none"""
    R = np.asarray(R, dtype=np.float64)
    ok = np.isfinite(R) & (R > 0)
    if not ok.any():
        return 1.0
    return float(f32(target / (2.0 * float(delta) * float(R[ok].max()))))


def clone(chk):
    """a second checker holding the same records, start indices, field, ids, channels and settings"""
    from tests.diffuse_ref import DiffuseChecker
    c = DiffuseChecker(chk.settings, chk.initial_offset, ref_quirks=chk.ref_quirks, channels=chk.channels)
    c.set_particles(chk.particles())
    c.start_indices_view()[:] = chk.start_indices_view()
    c.texture_view()[:] = chk.texture_view()
    c.ids, c.attr = chk.ids.copy(), chk.attr.copy()
    c.kappa, c.buoyancy, c.surface_tension = list(chk.kappa), chk.buoyancy, chk.surface_tension
    return c


def pass_of_next_step(chk, tick, stable=False):
    """What the pass of the next step will read and sum, on a clone (the keys, and with them the carry, depend on positions and
    velocities alone): {"attr": the carried channels, "R", "acc"}"""
    c = clone(chk)
    with np.errstate(all="ignore"):
        c.sorted_state(tick, stable)
        c.cell_starts(); c.density()
        _, _, R, acc = c.diffuse_pass()
    out = {"attr": c.attr.copy(), "R": R, "acc": acc}
    c.close()
    return out


def longest_row(keys):
    """the most candidates the sweep row of any particle holds (the cells id - 1 .. id + 1 of its own cell id: consecutive ids, as
    the kernels' row ranges are): a lower bound on the row range of that particle's block"""
    ids, cnt = np.unique(np.asarray(keys, dtype=np.int64), return_counts=True)
    tab = dict(zip(ids.tolist(), cnt.tolist()))
    return max(tab.get(i - 1, 0) + c + tab.get(i + 1, 0) for i, c in tab.items())


def channel_values(n):
    vals = H.sample_channel_values(n, 3)
    vals[0, 0], vals[0, 1] = f32(1.0), f32(-1.0)         # both signs of s even in a two-particle case
    return np.ascontiguousarray(np.concatenate([vals, special_bits(n)[None, :]]))


class Ref:
    """one checker step in the shape the GPU file compares: ids, channels, records, start indices, fb"""

    def __init__(self, chk):
        self.ids, self.attr, self.fb = chk.ids.copy(), chk.attr.copy(), None if chk.fb is None else chk.fb.copy()
        self.st = None if chk.st is None else chk.st.copy()
        self.rec, self.start = chk.particles(), chk.start_indices_view().copy()
        self.channels, self.n = self.attr.shape[0], self.ids.shape[0]

    def particles_view(self): return self.rec
    def start_indices_view(self): return self.start


class Run:
    pass


_RUNS = {}


def registry_run(fs, case, sort):
    """the case on the checker in the given sort mode, computed once: .steps (a Ref per step), .values (the uploaded channels),
    .kappa (per channel), and the figures .acc_share (the largest share, over the steps, of slots whose channel-0 sum is not +-0),
    .s_pos / .s_neg (slots, over all steps, with s = beta (A0 - a) above / below zero) and .longest_row (the most candidates any
    particle's sweep row holds: a lower bound on its block's row range)"""
    key = (case.name, sort)
    if key in _RUNS:
        return _RUNS[key]
    stable = sort == "counting"
    from tests.diffuse_ref import DiffuseChecker
    chk = DiffuseChecker(case.st, case.off, ref_quirks=case.quirks, channels=CHANNELS)
    chk.set_particles(case.start)
    if case.start_indices is not None:
        chk.start_indices_view()[:] = case.start_indices
    if case.field is not None:
        chk.texture_view()[:] = case.field
    run = Run()
    run.values = channel_values(case.n)
    chk.attr[:] = run.values
    k = kappa_for(pass_of_next_step(chk, case.tick, stable)["R"], case.tick.delta, 0.5)
    run.kappa = [k, 0.0, float(f32(4.0 * k)), k]
    chk.kappa = list(run.kappa)
    chk.buoyancy = (0, BETA, REFERENCE)
    run.steps, shares = [], []
    run.s_pos = run.s_neg = run.longest_row = 0
    with np.errstate(all="ignore"):
        for _ in range(case.steps):
            chk.step(case.tick, stable)
            s = f32(BETA) * (f32(REFERENCE) - chk.attr_in[0])
            run.s_pos += int((s > 0).sum()); run.s_neg += int((s < 0).sum())
            shares.append(float((chk.acc[0].view(np.uint32) << 1 != 0).mean()))
            run.longest_row = max(run.longest_row, longest_row(chk.particles_view()["grid"]))
            run.steps.append(Ref(chk))
    run.acc_share = max(shares)
    chk.close()
    _RUNS[key] = run
    return run
