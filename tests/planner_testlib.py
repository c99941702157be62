"""Helpers the planner tests share (tests/test_planner_cpu.py, tests/test_gpu_planner.py): the NumPy reference of the planner's
counter stream (on tests/counter_rng.py's Philox and Box-Muller), of the candidates and of MPPI's two-pass update in float64, and
the inputs both files must agree on.  A plain module: no fixtures, nothing registered with pytest."""
import numpy as np
import torch

from tests import returns_testlib as rt
from tests.counter_rng import MASK64, gauss_bound, gauss_pair, philox

MAX_N, MAX_C = 1 << 12, 1 << 17
GUMBEL_CODE = lambda i, q=0: i | 0x60000000 | (q << 12)       # fg_actor_rollout_kernel.hpp: actor_gumbel


def plan_code(c, i):
    """Counter word 1 of candidate c, agent i: top three bits 010."""
    return 0x40000000 | (c << 12) | i


def unit_draws(seed, env_index_base, C, K, B, N, noise_offset):
    """(eps [C,K,B,N,2] float64, r [C,K,B,N] the Box-Muller radius): step k draws at noise_offset + k (64-bit sum)."""
    c = np.arange(C, dtype=np.uint64)[:, None, None]
    g = np.broadcast_to(np.arange(B, dtype=np.uint64)[None, :, None] + np.uint64(env_index_base), (C, B, N))
    code = np.broadcast_to(np.uint64(0x40000000) | (c << np.uint64(12)) | np.arange(N, dtype=np.uint64)[None, None, :], (C, B, N))
    eps = np.empty((C, K, B, N, 2))
    for k in range(K):
        off = (int(noise_offset) + k) & MASK64
        w = philox(g, code, np.full((C, B, N), off & 0xFFFFFFFF, np.uint64), np.full((C, B, N), off >> 32, np.uint64), seed)
        eps[:, k] = gauss_pair(w[0], w[1])
    return eps, np.sqrt((eps ** 2).sum(-1))


def candidates64(mean, sigma, clip, eps):
    """clamp(mean + sigma eps) in float64: mean [K,B,N,2] (or None), eps [C,K,B,N,2]."""
    u = (0.0 if mean is None else np.asarray(mean, dtype=np.float64)[None]) + float(sigma) * eps
    return np.clip(u, -clip, clip) if clip > 0 else u


def mppi64(ret, u, lam):
    """The two-pass update in float64: ret [C,B,N], u [C,K,B,N,2] -> (new [K,B,N,2], abar [B,N] - the weight-averaged
    (m - ret_c) / lam -, umax [K,B,N] = max_c |u_c| over both components)."""
    ret = np.asarray(ret, dtype=np.float64)
    a = (ret.max(0, keepdims=True) - ret) / lam                   # [C,B,N] >= 0
    w = np.exp(-a)
    s = w.sum(0)
    new = (w[:, None, :, :, None] * u).sum(0) / s[None, :, :, None]
    return new, (w * a).sum(0) / s, np.abs(u).max(-1).max(0)


def mppi_bound(C, abar, umax, sigma, rmax):
    """Per (k, b, i) the bound of the fp32 update against mppi64 on the NumPy candidates: 2^-23 max|u| (C + 2 abar + 8) - the
    summations lose at most about C half-ulps in numerator and denominator, a weight's relative error is its argument's (two
    roundings, times the argument) plus the exponential's - plus the candidates' own sigma gauss_bound(r)."""
    return 2.0 ** -23 * umax * (C + 2.0 * abar[None] + 8.0) + sigma * gauss_bound(rmax)


def shifted(new):
    """What shift = 1 stores: row k at k - 1, the last row repeated."""
    return np.concatenate([new[1:], new[-1:]], 0) if isinstance(new, np.ndarray) else torch.cat([new[1:], new[-1:]], 0)


# ---- the inputs of "a small lambda picks the best candidate" (GPU) and of the CPU test that pins them ----
PICK = dict(N=3, B=24, C=8, K=3, seed=rt.SEED, noise_offset=11, sigma=0.7, clip=1.0, lam=1e-4, gamma=0.97)
GAP_FACTOR = 150.0                  # a runner-up this many lam below the best has weight exp(-150): zero in fp32


def pick_mean(d=PICK):
    """The plan's mean [K,B,N,2] fp32 in [-0.5, 0.5) of the pick test (CPU tensor)."""
    g = torch.Generator().manual_seed(31 * d["seed"] + 7)
    return torch.rand((d["K"], d["B"], d["N"], 2), generator=g) - 0.5


def pick_state(d=PICK):
    """The state of the pick test as `oracle_returns` takes it, every value fp32-representable (the env is given exactly these)."""
    st = rt.oracle_state(d["B"], d["N"], d["K"], seed=d["seed"])
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    return dict(pos=st["pos"], vel=st["vel"], ideal_shape=f32(st["ideal_shape"]), ideal_vel=f32(st["ideal_vel"]), step=st["step"])


def pick_oracle(d=PICK):
    """(best [B] candidate index, gap [B] between the best and the runner-up shared return, margin [C,B]) in float64 on the
    NumPy candidates rounded to fp32 (the device's candidates are within gauss_bound of them)."""
    eps, _ = unit_draws(d["seed"], 0, d["C"], d["K"], d["B"], d["N"], d["noise_offset"])
    u = candidates64(pick_mean(d).double().numpy(), d["sigma"], d["clip"], eps)
    shared, _, _, margin = rt.oracle_returns(pick_state(d), u, d["gamma"])
    r = shared[:, :, 0]                                            # the shared return is one number per (candidate, env)
    order = np.sort(r, 0)
    return r.argmax(0), order[-1] - order[-2], margin
