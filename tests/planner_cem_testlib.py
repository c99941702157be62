"""Helpers the CEM planner tests share (tests/test_planner_cem_cpu.py, tests/test_gpu_planner_cem.py): the NumPy reference of
`fg_plan_cem_update`'s selection (the total order on the bits, ties by the lower index), of the candidates with a sigma tensor and
of the refit in float64, the refit's error bound, and the synthetic return rows the selection is tried on.  On
tests/planner_testlib.py's draws.  A plain module: no fixtures, nothing registered with pytest."""
import numpy as np

from tests import planner_testlib as pt
from tests.counter_rng import gauss_bound

EPS = 2.0 ** -23                                           # one fp32 ulp of 1: twice the unit roundoff


# ---- the selection ----
def keys(ret):
    """The uint32 sort key of fp32 values: bits ^ (sign ? 0xFFFFFFFF : 0x80000000) - a total order on every bit pattern."""
    bits = np.ascontiguousarray(ret, dtype=np.float32).view(np.uint32)
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def select(ret, E):
    """ret [C, ...] fp32 -> [E, ...] int32: per column the indices of the E largest keys, equal keys the lower index first, in
    ascending order (what `elite_idx` holds)."""
    order = np.argsort(~keys(ret), axis=0, kind="stable")            # descending keys; stable: ties keep ascending c
    return np.sort(order[:E], axis=0).astype(np.int32)


# ---- the synthetic rows of the selection test: pattern(C, rng) -> [C] fp32 ----
def _with_infs(C, rng):
    x = rng.standard_normal(C).astype(np.float32)
    x[0], x[-1] = -np.inf, np.inf                          # (C = 1: +inf alone)
    return x


PATTERNS = (
    ("distinct", lambda C, rng: (rng.permutation(C) - C / 2.0).astype(np.float32) * np.float32(0.37)),
    ("all equal", lambda C, rng: np.full(C, -3.5, np.float32)),
    ("ties straddle the threshold", lambda C, rng: rng.integers(0, 3, C).astype(np.float32) - np.float32(200.0)),
    ("mixed signs with both zeros", lambda C, rng: rng.choice(np.array([-2.5, -1.0, -0.0, 0.0, 1.0, 2.5], np.float32), C)),
    ("-inf and +inf", _with_infs),
    ("descending", lambda C, rng: -np.arange(C, dtype=np.float32)),
    ("ascending", lambda C, rng: np.arange(C, dtype=np.float32)),
)


def pattern_rows(C, first, rows, seed=0):
    """[C, rows] fp32: column j is pattern (first + j) mod 7."""
    rng = np.random.default_rng(1000 * C + seed)
    return np.stack([PATTERNS[(first + j) % len(PATTERNS)][1](C, rng) for j in range(rows)], 1)


def elite_counts(C, cap):
    """The E at which the selection is tried for C candidates: 1, 2, C / 2, C - 1, C, and the elite list's cap and one above."""
    return sorted({e for e in (1, 2, C // 2, C - 1, C, cap, cap + 1) if 1 <= e <= C})


# ---- the candidates and the refit in float64 ----
def candidates64_std(mean, std, clip, eps):
    """clamp(mean + std eps) in float64: mean (or None), std [K,B,N,2], eps [C,K,B,N,2]."""
    u = (0.0 if mean is None else np.asarray(mean, dtype=np.float64)[None]) + np.asarray(std, dtype=np.float64)[None] * eps
    return np.clip(u, -clip, clip) if clip > 0 else u


def gather_elites(x, elite):
    """x [C,K,B,N,...] and elite [E,B,N] -> [E,K,B,N,...]."""
    idx = elite.astype(np.int64)[:, None]                                      # [E,1,B,N]
    idx = idx.reshape(idx.shape + (1,) * (x.ndim - 4))
    return np.take_along_axis(x, np.broadcast_to(idx, (elite.shape[0],) + x.shape[1:]), 0)


def cem64(u, elite, mean_in, std_in, alpha, sigma_min):
    """The refit in float64 (shift 0): u [C,K,B,N,2], elite [E,B,N] -> (mean_new, std_new, m, s) [K,B,N,2] with m the elites'
    mean and s their population standard deviation (centred, two passes)."""
    ue = gather_elites(u, elite)
    m = ue.mean(0)
    s = np.sqrt(((ue - m[None]) ** 2).mean(0))
    mean_in, std_in = np.asarray(mean_in, np.float64), np.asarray(std_in, np.float64)
    return (1.0 - alpha) * mean_in + alpha * m, np.maximum(sigma_min, (1.0 - alpha) * std_in + alpha * s), m, s


def cem_bound(u, eps, r, elite, mean_in, std_in, alpha, m, s):
    """(mean_bound, std_bound) [K,B,N,2] of the fp32 refit against cem64 on the NumPy candidates, with h = 2^-24 the unit roundoff
    (EPS = 2 h).  Everything is taken over a row's elites.

    The candidates.  The device's u is fl(mean + fl(std eps32)), clamped, with |eps32 - eps| <= gauss_bound(r): against the
    float64 candidate it is off by at most
        e_u = max std gauss_bound(r) + EPS amax,      amax = max(|mean| + std |eps|)
    (the draw, then one rounding of the product and one of the sum; the clamp is 1-Lipschitz).
    The mean.  The kernel forms dm = (sum fl(u - mean_in)) / E - per-lane sums, one butterfly: no more than E - 1 additions on any
    path - and m = fl(mean_in + dm), mean_new = fl(mean_in + alpha dm).  With D = max|u - mean_in| <= 2 umax, umax = max(|u|,
    |mean_in|): each difference is off by h D, the sum by (E - 1) h E D, the division by h D: together, over E, h D (E + 1)
    <= EPS umax (E + 1); the final product and sum add EPS (|mean_in| + D) <= 3 EPS umax:
        e_m       = EPS umax (E + 6) + e_u                       (the elites' mean m, alpha = 1; 2 umax of slack)
        mean_bound = alpha (EPS umax (E + 3) + e_u) + 3 EPS umax <= e_m     - alpha's rounding is the 3 EPS umax.
    The variance.  d = fl(u - m) is off by e_d = e_u + e_m + h Dm with Dm = max|u - m| + e_u + e_m (the fp32 deviations' own
    size); a square by 2 Dm e_d + h Dm^2, the sum of E squares by (E - 1) h E Dm^2, the division by h Dm^2: over E
        e_v = EPS Dm^2 (E + 4) / 2 + 2 Dm (e_u + e_m).
    The standard deviation.  |sqrt(a) - sqrt(b)| = |a - b| / (sqrt(a) + sqrt(b)) <= e_v / s64 - the issue's quotient with the
    fp32 root dropped from the denominator, so that the bound does not read the result it judges - and always <= sqrt(|a - b|):
        e_s = e_v / s64  where s64^2 >= e_v,  sqrt(e_v) below it - the switch is at a variance equal to its own error, where
    the variance is ill-conditioned.  The hardware square root adds EPS s, the convex sum (1 - alpha) std_in + alpha s (fl(1 -
    alpha), two products, one sum) 2 EPS (std_in + s); max(sigma_min, .) is 1-Lipschitz:
        std_bound = alpha (e_s + EPS s64) + 2 EPS (std_in + s64 + e_s)."""
    E = elite.shape[0]
    mean_in, std_in = np.asarray(mean_in, np.float64), np.asarray(std_in, np.float64)
    ue = gather_elites(u, elite)
    amax = (np.abs(mean_in)[None] + std_in[None] * np.abs(gather_elites(eps, elite))).max(0)
    gb = gauss_bound(gather_elites(r, elite).max(0))[..., None]
    e_u = std_in * gb + EPS * amax
    umax = np.maximum(np.abs(ue).max(0), np.abs(mean_in))
    e_m = EPS * umax * (E + 6) + e_u
    mean_bound = alpha * (EPS * umax * (E + 3) + e_u) + 3 * EPS * umax
    Dm = np.abs(ue - m[None]).max(0) + e_u + e_m
    e_v = EPS * Dm ** 2 * (E + 4) / 2 + 2 * Dm * (e_u + e_m)
    e_s = np.where(s ** 2 >= e_v, e_v / np.maximum(s, 1e-300), np.sqrt(e_v))
    std_bound = alpha * (e_s + EPS * s) + 2 * EPS * (std_in + s + e_s)
    return mean_bound, std_bound


shifted = pt.shifted
