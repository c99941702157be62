"""The fp64 reference, actor builders, bounds, inputs and reference mutants the Gumbel-softmax actor tests share
(tests/test_actor_gumbel_cpu.py, tests/test_gpu_actor_gumbel.py).  A plain module, device-agnostic; no fixtures, nothing
registered with pytest.

The semantics (one definition: csrc/fg_actor_rollout_kernel.hpp `actor_gumbel`, `gumbel_pick`, `cat_decode`).  Per (env b, agent
i, step k) the actor gives five logits l_0..l_4.  The five Gumbel draws come from a Philox4x32-10 stream of their own - key
`seed`, counter {b + env_index_base, i | 0x60000000 | (q << 12), lo32(off), hi32(off)}, off = rng_base + k; draw j is word j & 3
of block q = j >> 2 - as u_j = (2 (c >> 9) + 1) 2^-24 (an odd 24-bit integer scaled: exact in fp32, strictly inside (0, 1)) and
g_j = -log(-log(u_j)).  Exploring, y_j = l_j + g_j; otherwise y_j = l_j; the index is the lowest j attaining max_j y_j and
becomes the raw action by the env's action mode (`actor_cat_testlib.decode`).  Everything here is NumPy fp64, written by hand.

Bounds (derived, not measured).  With a logarithm good to 2 ulp the inner one carries 2^-22 relative, which is 2^-22 absolute on
the outer one, whose own rounding is 2^-22 |g|: a device draw lies within
    gamma_j = 2^-21 (1 + max(1, |g_j|))
of this reference on the same u_j (at most 8.9e-6, at the extreme draw g = 16.64).  A kernel's fp32 logits differ from the fp64
ones by at most the row's logit bound beta - `actor_cat_testlib.TOL` max(1, max_j |l_j|), times max(1, s) behind a BatchNorm
(`actor_bn_testlib.bn_scale`) - so its y_j differs from the reference's by at most beta + gamma_j plus the sum's rounding, 2^-19
while |y| < 64.  A row may therefore pick another index only where the gap between its two largest y_j is at most
    eta = 2 beta + 2 max_j gamma_j + 2^-17        (exploring);        eta = 2 beta        (not exploring, y = l).
`pick` returns that gap as each row's margin and `exempt` applies the band.  The band may hold at most EXEMPT_CAP = 1 % of a
case's rows: tests/test_actor_gumbel_cpu.py shows that the reference alone meets it on `CASES` and that max |y| < 64 there.

Mutants.  `MUTANTS` names the reference with exactly one deliberate error each; `gumbels` / `launch_gumbels` / `pick` /
`logits64` take the mutant's name and `actor_cat_testlib.decode` the one of the decode.  tests/test_actor_gumbel_cpu.py shows
that each differs from the true reference in a stated share of the values the GPU tests compare.
"""
import copy

import numpy as np
import torch

from formation_gym import GumbelSoftmaxActor, InputBatchNorm, PerAgentActor
from tests import actor_bn_testlib as bt
from tests import actor_cat_testlib as ct
from tests import counter_rng as R

nn = torch.nn
ONEHOT5, INDEX, ARGMAX = ct.ONEHOT5, ct.INDEX, ct.ARGMAX
TOL = ct.TOL
SUM_ROUNDING = 2.0 ** -17                              # both sums' rounding, 2^-19 each while |y| < 64, with room
Y_MAX = 64.0
EXEMPT_CAP = 0.01

SEED, BASE, K, OFFSET = ct.SEED, ct.BASE, ct.K, ct.OFFSET
# N x B: 3 x 70 - E = 64, a second workgroup with 6 live envs; 4 x 70 - the group's lanes exactly full; 9 x 20 - a half-empty
# last pass; 27 x 11 - half-full agent-major tiles; 32 x 9 - the last slot of the per-agent table
SHAPES = ((3, 70), (4, 70), (9, 20), (27, 11), (32, 9))
FORMS = ("plain", "pa", "bn", "pa_bn")                 # shared / per agent, without / behind the input BatchNorm
_ONE_MODE = {(3, 70): ONEHOT5, (4, 70): INDEX, (27, 11): ONEHOT5, (32, 9): INDEX}


def _modes(n, b):
    return (ONEHOT5, INDEX) if (n, b) == (9, 20) else (_ONE_MODE[(n, b)],)


# (form, N, B, H, mode): H = 64 for the four forms at every shape, H = 32 at 9 x 20 and 27 x 11, H = 128 once each for the
# forms without a BatchNorm at 3 x 70; both modes at 9 x 20, one elsewhere
CASES = [(f, n, b, 64, m) for f in FORMS for (n, b) in SHAPES for m in _modes(n, b)] \
    + [(f, n, b, 32, m) for f in FORMS for (n, b) in ((9, 20), (27, 11)) for m in _modes(n, b)] \
    + [(f, 3, 70, 128, ONEHOT5) for f in ("plain", "pa")]

MUTANTS = ("actor_stream", "blocks_swapped", "draw4_word3_block0", "shift8_no_half", "offset_not_advanced", "base_dropped",
           "noise_dropped", "noise_when_not_exploring", "highest_tie", "modes_swapped", "head_rows_agent0")


# ---- the reference ----
def stream_code(i, q=0):
    """Counter word 1 of block q of agent i's Gumbel draws: top three bits 011 for i < 2^12."""
    return i | 0x60000000 | (q << 12)


def u_of(word, mutant=None):
    """u in (0, 1) of a 32-bit Philox word, fp64 (exactly representable in fp32)."""
    w = np.asarray(word, dtype=np.uint64)
    if mutant == "shift8_no_half":
        return (w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    return (2.0 * (w >> np.uint64(9)).astype(np.float64) + 1.0) * 2.0 ** -24


def gumbel_of(u):
    with np.errstate(divide="ignore"):
        return -np.log(-np.log(np.asarray(u, dtype=np.float64)))


def gumbels(seed, base, B, N, offset, mutant=None):
    """g [B, N, 5] fp64 of one step at counter offset `offset` (already rng_base + k)."""
    v = R.Variant(use_base=False) if mutant == "base_dropped" else R.TRUE
    code = (lambda i, q: R.STREAM_CODES["actor_noise"](i)) if mutant == "actor_stream" else stream_code
    q0, q1 = (1, 0) if mutant == "blocks_swapped" else (0, 1)
    c0 = R.blocks(seed, base, B, [code(i, q0) for i in range(N)], offset, v)
    c1 = R.blocks(seed, base, B, [code(i, q1) for i in range(N)], offset, v)
    words = [c0[0], c0[1], c0[2], c0[3], c0[3] if mutant == "draw4_word3_block0" else c1[0]]
    return gumbel_of(np.stack([u_of(w, mutant) for w in words], -1))


def launch_gumbels(seed, base, B, N, rbase, steps, mutant=None):
    """g [steps, B, N, 5] of a launch whose base offset is rbase: step k at rbase + k (64-bit wrap-around)."""
    adv = mutant != "offset_not_advanced"
    return np.stack([gumbels(seed, base, B, N, (int(rbase) + (k if adv else 0)) & R.MASK64, mutant) for k in range(steps)])


def gamma(g):
    """The per-draw bound of a device draw against `gumbels` (module docstring)."""
    return 2.0 ** -21 * (1.0 + np.maximum(1.0, np.abs(np.asarray(g, dtype=np.float64))))


def pick(logits, g=None, explore=True, mutant=None):
    """(idx int64 [...], margin [...]) of logits [..., 5] (fp64) and draws g [..., 5]: the lowest index of the largest y_j, and
    the gap between the two largest y_j."""
    l = np.asarray(logits, dtype=np.float64)
    add = (explore and mutant != "noise_dropped") or (not explore and mutant == "noise_when_not_exploring")
    y = l + np.asarray(g, dtype=np.float64) if add else l
    m = y.max(-1, keepdims=True)
    idx = np.where(y == m, np.arange(5), -1).max(-1) if mutant == "highest_tie" else np.where(y == m, np.arange(5), 5).min(-1)
    srt = np.sort(y, -1)
    return idx.astype(np.int64), srt[..., 4] - srt[..., 3]


decode = ct.decode


def eta(beta, g=None, explore=True):
    """The band of the module docstring for rows of logit bound beta [...] and draws g [..., 5]."""
    if not explore:
        return 2.0 * np.asarray(beta)
    return 2.0 * np.asarray(beta) + 2.0 * gamma(g).max(-1) + SUM_ROUNDING


def exempt(margin, beta, g=None, explore=True, scale=1.0):
    """Rows a kernel may pick differently: margin <= scale eta."""
    return margin <= scale * eta(beta, g, explore)


# ---- builders: the Gumbel-softmax actors of the four fused forms ----
def _member(N, H, seed, bn, norm, eps=1e-5, affine=True):
    """One logits network on the CPU: `actor_cat_testlib`'s plain body with its five-output head (PyTorch's default
    initialisation under `seed`, times ACT_SCALE, the head times HEAD_SCALE on top), behind `actor_bn_testlib.bn_actor`'s
    BatchNorm of the same seed when `bn`."""
    body = list(ct.cat_actor("plain", N, H, seed=seed).logits)
    if bn:
        body = [bt.bn_actor(N, H, seed=seed, eps=eps, affine=affine, norm=norm)[0]] + body
    return nn.Sequential(*body).eval()


def gumbel_actor(form, N, H, seed=0, device=None, explore=True, identical=False, head=5, tanh=False):
    """GumbelSoftmaxActor over the `form` logits - 'plain' / 'bn': one shared network, without / behind an InputBatchNorm; 'pa'
    / 'pa_bn': a PerAgentActor of N members (nn.BatchNorm1d norms: members see 2-D rows) with distinct weights and, 'pa_bn',
    statistics, eps cycling over 1e-5, 1e-3, 1e-2 and every third member without affine parameters - or, `identical`, N copies
    of the shared form's network.  `head` / `tanh`: another head width, a Tanh after it (forms the rule must refuse)."""
    bn = form in ("bn", "pa_bn")
    if form in ("plain", "bn"):
        logits = _member(N, H, seed, bn, InputBatchNorm)
    elif identical:
        logits = PerAgentActor([_member(N, H, seed, bn, nn.BatchNorm1d) for _ in range(N)])
    else:
        logits = PerAgentActor([_member(N, H, seed + 7 * i, bn, nn.BatchNorm1d, (1e-5, 1e-3, 1e-2)[i % 3], i % 3 != 2)
                                for i in range(N)])
    if head != 5 or tanh:
        for m in ([logits] if form in ("plain", "bn") else logits.actors):
            if head != 5:
                m[-1] = nn.Linear(H, head)
            if tanh:
                m.append(nn.Tanh())
    actor = GumbelSoftmaxActor(logits.eval(), explore)
    return actor if device is None else actor.to(device)


def logits64(actor64, form, obs, mutant=None):
    """(logits [..., N, 5], beta [..., N]) of the fp64 copy `actor64` of a `gumbel_actor` on observations obs [..., N, 6N], as
    NumPy fp64; beta is the row's logit bound (module docstring; agent i's own BatchNorm scale for a per-agent form).
    `mutant` 'head_rows_agent0': every agent's head rows (w3, b3) taken from agent 0's network."""
    bn = form in ("bn", "pa_bn")
    with torch.no_grad():
        if form in ("plain", "bn"):
            lg = actor64.logits(obs)
            fac = torch.full_like(lg[..., 0], max(1.0, bt.bn_scale(actor64.logits[0])) if bn else 1.0)
        else:
            members = list(actor64.logits.actors)
            head0 = members[0][-1]
            rows = []
            for i, m in enumerate(members):
                x = obs[..., i, :]
                rows.append(head0(m[:-1](x)) if mutant == "head_rows_agent0" else m(x))
            lg = torch.stack(rows, dim=-2)
            fac = torch.ones_like(lg[..., 0])
            if bn:
                for i, m in enumerate(members):
                    fac[..., i] = max(1.0, bt.bn_scale(m[0]))
        beta = TOL * torch.clamp(lg.abs().max(-1).values, min=1.0) * fac
    return lg.cpu().numpy(), beta.cpu().numpy()


def double(actor):
    """The fp64 copy of a `gumbel_actor` (eval mode kept)."""
    return copy.deepcopy(actor).double().eval()


cpu_observations = ct.cpu_observations


# ---- the standalone fg_actor_gumbel_pick inputs (GPU test 2) ----
G_MIN = float(gumbel_of(2.0 ** -24))                   # the extreme draws: c >> 9 = 0 and 2^23 - 1
G_MAX = float(gumbel_of(1.0 - 2.0 ** -24))


def standalone_inputs(seed=5, rows=4096):
    """(logits fp32 [rows, 5], g fp32 [rows, 5]): normal logits of several scales and Gumbel draws of random words, then the edge
    rows - a tie of two maxima (1 and 4) and of three (0, 2, 3) in the logits with equal draws there, so that y ties exactly
    whether or not the launch explores; one logit at +100 against -100; one logit at -100; and the two extreme draws cycled
    over the columns of every kind of row."""
    rng = np.random.RandomState(seed)
    lg = (rng.standard_normal((rows, 5)) * rng.choice([0.3, 1.0, 3.0, 8.0], (rows, 1))).astype(np.float32)
    g = gumbel_of(u_of(rng.randint(0, 1 << 32, (rows, 5), dtype=np.uint64))).astype(np.float32)
    col = np.arange(rows) % 5
    g[5::7, :] = np.float32(0.5)
    g[np.arange(rows)[5::7], col[5::7]] = np.float32(G_MAX)
    g[np.arange(rows)[6::7], col[6::7]] = np.float32(G_MIN)
    lg[1::64] = -100.0; lg[1::64, 3] = 100.0              # one logit at +100 against -100: no draw reaches it
    lg[4::64, 2] = -100.0                                 # one logit at -100: never taken
    top = np.abs(lg[2::64]).max(-1) + np.float32(30.0)    # a tie of two maxima (1 and 4), beyond every draw's reach
    lg[2::64, 1] = top; lg[2::64, 4] = top
    g[2::64, 1] = g[2::64, 4] = np.float32(0.25)
    lg[3::64, 0] = lg[3::64, 2] = lg[3::64, 3] = 40.0     # a tie of three
    lg[3::64, 1] = lg[3::64, 4] = -2.0
    g[3::64, 0] = g[3::64, 2] = g[3::64, 3] = np.float32(1.5)
    return lg, g
