"""How the hard-input registries (tests/features2d.py, tests/features3d.py) choose a case's surface-tension coefficient and
threshold: from the case's CPU checker alone, never from the engine.  TEST INFRASTRUCTURE, plain numpy, no GPU."""
import numpy as np

f32 = np.float32


def median_pos(x):
    x = np.asarray(x, dtype=np.float64)
    x = x[np.isfinite(x) & (x > 0)]
    return float(np.median(x)) if x.size else 0.0


def gap_threshold(nl):
    """a threshold near the median of the finite, non-zero |n| values, in the widest relative gap of their middle half (as
    test_tolerance_mode_within_tolerance places it); 0 when fewer than two such values exist"""
    nl = np.sort(np.asarray(nl, dtype=np.float64))
    nl = nl[np.isfinite(nl) & (nl > 0)]
    if nl.size < 2:
        return 0.0
    mid = nl[nl.size // 4: max(3 * nl.size // 4, nl.size // 4 + 2)]
    k = int(np.argmax(mid[1:] / mid[:-1]))
    return float(f32(np.sqrt(mid[k] * mid[k + 1])))


def choose_surface_tension(case, own, tension, delta):
    """sigma: the ratio of the medians of the step's own acceleration (`own()`: per particle, the plain step on the checker) and of
    |st| / rho at sigma = 1 (`tension(1.0)[0]`), so that the pass changes velocities by as much as the step does; kept inside
    [1e-30, 1e30] and 1 where the pass gives no finite force.  tau: gap_threshold of the |n| of one step with (sigma, 0),
    `tension(sigma)[1]`.  Sets case.sigma, case.tau and the figures of the choice."""
    with np.errstate(all="ignore"):
        a = median_pos(own())
        b = median_pos(tension(1.0)[0])
        sigma = float(f32(min(max(a / b, 1e-30), 1e30))) if a > 0 and b > 0 else 1.0
        unit, nl = tension(sigma)
        tau = gap_threshold(nl)
        dv = np.asarray(unit, dtype=np.float64) * float(delta)
    pos = np.isfinite(nl) & (nl > 0)
    case.sigma, case.tau = sigma, tau
    case.figures.update(sigma=sigma, tau=tau, n=int(nl.shape[0]), with_n=int(pos.sum()), above=int((pos & (nl > f32(tau))).sum()),
                        below=int((pos & ~(nl > f32(tau))).sum()), own_dv=a * float(delta), st_dv=median_pos(dv))
    return case
