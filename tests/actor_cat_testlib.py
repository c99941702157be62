"""The fp64 reference, actor builders, bounds, inputs and reference mutants the categorical actor tests share
(tests/test_actor_categorical_cpu.py, tests/test_gpu_actor_categorical.py).  A plain module, device-agnostic; no fixtures,
nothing registered with pytest.

The semantics (one definition: csrc/fg_actor_rollout_kernel.hpp `cat_pick`, `actor_uniform`, `cat_decode`).  Per (env b, agent
i, step k) the actor gives five logits l_0..l_4.  The uniform draw is word 2 of the Philox4x32-10 block the Gaussian members
draw for (b, i, k) - key `seed`, counter {b + env_index_base, i ^ 0xA0000000, lo32(off), hi32(off)}, off = rng_base + k - as
u = (c[2] >> 8) 2^-24 in [0, 1), exact in fp32.  Then
    m = max_j l_j,  e_j = exp(l_j - m),  c_j = e_0 + .. + e_j (ascending),  s = c_4
    sampled: t = u s, idx the first j in 0..3 with t < c_j, else 4;     greedy: idx the lowest index attaining m
    log_prob = (l_idx - m) - log(s)
and the index becomes the raw action by the env's action mode: FG_ACT_ONEHOT5 0 -> (0,0), 1 -> (+1,0), 2 -> (-1,0), 3 -> (0,+1),
4 -> (0,-1); FG_ACT_INDEX 1 -> (-1,0), 2 -> (+1,0), 3 -> (0,-1), 4 -> (0,+1).  Everything here is NumPy fp64, written by hand.

Exemption band.  A kernel's fp32 logits differ from the fp64 ones by at most the row's logit bound beta (the family's action
bound with |a| replaced by max_j |l_j|).  A log-softmax moves by at most 2 beta (the logit and the log-sum-exp each by beta) and
a CDF value c_j / s by at most as much again, so a row may pick another index only where |u s - c_j| <= eta s for some j < 4,
eta = 4 beta + 2^-16; the 2^-16 covers the fp32 exp, the four additions and the product u s (a few 2^-22 each, c_j / s <= 1).
`pick` returns each row's margin min_j |u s - c_j| / s so that a test can apply the band.

Mutants.  `MUTANTS` names the reference with exactly one deliberate error each; `pick` / `uniform` / `decode` take the mutant's
name.  tests/test_actor_categorical_cpu.py shows that each differs from the true reference in a stated share of the values the
GPU tests compare, on `CASES`' shapes and the seeds below, with logits of the builders' distribution.
"""
import numpy as np
import torch

from formation_gym import CategoricalActor, RecurrentActor
from tests import counter_rng as R
from tests.actor_fidelity import _body, _norm, _per_norm, _perturb_norm
from tests.actor_testlib import ACT_SCALE

nn = torch.nn
ONEHOT5, INDEX, ARGMAX = 1, 2, 3
TOL = 1e-5                                             # the families' action bound: TOL max(1, |a|) [rstd factors]
ETA0 = 2.0 ** -16
# the head's parameters times this, per family: per-row max probabilities from ~0.25 (near-uniform) to > 0.9
HEAD_SCALE = {"plain": 8.0, "ln": 6.0, "gru": 6.0}
# eps of every LayerNorm of the builders: rstd <= 1 / sqrt(eps) = 1.41, so the rstd factors of the LayerNorm families' bounds
# stay near 1 and the exemption band (eta = 4 beta + 2^-16) takes well under 2 % of the rows
NORM_EPS = 0.5

# the GPU tests' inputs: env_index_base, a 64-bit seed, an offset whose K = 3 steps cross 2^32 (tests/counter_rng.py's)
SEED = R.SEED
BASE = R.BASE
K = 3
OFFSET = 2 ** 32 - 2
# (family, N, B, H): N = 3 x 70 - E = 64, a second workgroup with 6 live envs; 9 x 20 - E = 16, 180 rows, a half-empty last
# 32-row pass in the tail workgroup; 27 x 11 - E = 8, 6.75 passes; H = 128 once, plain at N = 3
SHAPES = ((3, 70), (9, 20), (27, 11))
CASES = [(fam, n, b, h) for fam in ("plain", "ln", "gru") for (n, b) in SHAPES for h in (32, 64)] + [("plain", 3, 70, 128)]

# the builders' seed per case: 0, and 1 where seed 0's actor leaves no near-uniform row (ln 9 x 20, H = 32: smallest max
# probability 0.44) or never picks index 3 (gru 3 x 70, H = 32) on the reference's inputs - test_actor_categorical_cpu.py
# checks both properties for every case at the seed used
CASE_SEED = {("ln", 9, 20, 32): 1, ("gru", 3, 70, 32): 1}


def case_seed(fam, N, B, H):
    return CASE_SEED.get((fam, N, B, H), 0)


MUTANTS = ("word0", "word3", "offset_not_advanced", "base_dropped", "modes_swapped", "axes_swapped", "t_is_u",
           "descending_cumsum", "greedy_highest_tie", "logp_of_greedy")


# ---- the reference ----
def uniform(seed, base, B, N, offset, mutant=None):
    """u [B, N] fp64 of one step at counter offset `offset` (already rng_base + k)."""
    v = R.Variant(use_base=False) if mutant == "base_dropped" else R.TRUE
    c = R.blocks(seed, base, B, [R.STREAM_CODES["actor_noise"](i) for i in range(N)], offset, v)
    word = {"word0": 0, "word3": 3}.get(mutant, 2)
    return (c[word] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def launch_uniforms(seed, base, B, N, rbase, steps, mutant=None):
    """u [steps, B, N] of a launch whose base offset is rbase: step k at rbase + k (64-bit wrap-around)."""
    adv = mutant != "offset_not_advanced"
    return np.stack([uniform(seed, base, B, N, (int(rbase) + (k if adv else 0)) & R.MASK64, mutant) for k in range(steps)])


def pick(logits, u=None, greedy=False, mutant=None):
    """(idx int64 [...], log_prob [...], margin [...]) of logits [..., 5] (fp64) and draws u [...]; margin = min_{j<4}
    |u s - c_j| / s when sampling, the top-two logit gap when greedy."""
    l = np.asarray(logits, dtype=np.float64)
    m = l.max(-1, keepdims=True)
    e = np.exp(l - m)
    if mutant == "descending_cumsum":
        c = np.cumsum(e[..., ::-1], -1)
    else:
        c = np.cumsum(e, -1)
    s = c[..., 4]
    srt = np.sort(l, -1)
    top = np.where(l == m, np.arange(5), 5).min(-1)
    if mutant == "greedy_highest_tie":
        top = np.where(l == m, np.arange(5), -1).max(-1)
    if greedy:
        idx, margin = top, srt[..., 4] - srt[..., 3]
    else:
        t = np.asarray(u, dtype=np.float64) * (1.0 if mutant == "t_is_u" else s)
        idx = (t[..., None] >= c[..., :4]).sum(-1)      # the first j with t < c_j, else 4 (c ascending)
        margin = np.abs(t[..., None] - c[..., :4]).min(-1) / s
    at = top if (mutant == "logp_of_greedy" and not greedy) else idx
    logp = np.take_along_axis(l - m, at[..., None], -1)[..., 0] - np.log(s)
    return idx.astype(np.int64), logp, margin


_TABLE = {ONEHOT5: np.array([[0, 0], [1, 0], [-1, 0], [0, 1], [0, -1]], dtype=np.float64),
          INDEX: np.array([[0, 0], [-1, 0], [1, 0], [0, -1], [0, 1]], dtype=np.float64)}


def decode(mode, idx, mutant=None):
    """The raw action [..., 2] of the indices in the action mode."""
    if mutant == "modes_swapped":
        mode = INDEX if mode == ONEHOT5 else ONEHOT5
    u = _TABLE[mode][np.asarray(idx)]
    return u[..., ::-1].copy() if mutant == "axes_swapped" else u


def exempt(margin, beta):
    """Rows a kernel may pick differently: margin <= 4 beta + 2^-16 (module docstring)."""
    return margin <= 4.0 * np.asarray(beta) + ETA0


# ---- builders: the categorical actors of the three fused forms ----
def _scale_head(lin, family):
    with torch.no_grad():
        for p in lin.parameters():
            p.mul_(HEAD_SCALE[family])


def cat_actor(family, N, H, seed=0, in_norm=True, device=None, deterministic=False, head=5, norm_eps=None):
    """CategoricalActor over the `family` body - 'plain': Linear, ReLU, Linear, ReLU, Linear(H, 5); 'ln': the MAPPO body with
    LayerNorms; 'gru': a RecurrentActor on that body - PyTorch's default initialisation under `seed`, the body's Linears (and
    the GRU) times ACT_SCALE, gamma / beta away from 1 / 0, the head times HEAD_SCALE[family] on top; every LayerNorm's eps is NORM_EPS, or
    `norm_eps` (1e-5: the trainers' default, for cases that need no exemption band)."""
    torch.manual_seed(seed)
    D = 6 * N
    lin = nn.Linear(H, head)
    if family == "plain":
        logits = nn.Sequential(nn.Linear(D, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), lin)
    else:
        eps = NORM_EPS if norm_eps is None else norm_eps
        one = _per_norm(eps), _per_norm(True), _per_norm(True)
        mods = _body(N, H, in_norm, one[0], one[1], one[2], True)
        if family == "ln":
            logits = nn.Sequential(*(mods + [lin]))
        else:
            logits = RecurrentActor(nn.Sequential(*mods), nn.GRUCell(H, H), _norm(H, eps, True, True), lin)
    with torch.no_grad():
        for mod in logits.modules():
            if isinstance(mod, (nn.Linear, nn.GRUCell)):
                for p in mod.parameters():
                    p.mul_(ACT_SCALE)
            elif isinstance(mod, nn.LayerNorm):
                _perturb_norm(mod)
    _scale_head(lin, family)
    actor = CategoricalActor(logits, deterministic)
    return actor if device is None else actor.to(device)


def logits64(actor64, family, obs, h=None):
    """(logits [..., 5], beta [...], new state or None, state bound [..., 1] or None) of the fp64 copy `actor64` of a `cat_actor` on observations obs
    (and GRU states h), as NumPy fp64: beta is the row's logit bound - the family's action bound with max_j |l_j| for |a| - and the state bound the
    recurrent family's per-row TOL max(1, r1) max(1, r2) (tests/actor_fidelity.py rec_bounds)."""
    from tests.actor_fidelity import ln_ref64, rec_ref64
    with torch.no_grad():
        if family == "plain":
            lg = actor64.logits(obs)
            fac, hn, hb = torch.ones_like(lg[..., :1]), None, None
        elif family == "ln":
            lg, r1, r2, _ = ln_ref64(actor64.logits, obs)
            fac, hn, hb = torch.clamp(r1, min=1.0) * torch.clamp(r2, min=1.0), None, None
        else:
            lg, hn, r1, r2, r3 = rec_ref64(actor64.logits, obs, h)
            hb = TOL * torch.clamp(r1, min=1.0) * torch.clamp(r2, min=1.0)
            fac = torch.clamp(r1, min=1.0) * torch.clamp(r2, min=1.0) * torch.clamp(r3, min=1.0)
        beta = TOL * torch.clamp(lg.abs().max(-1).values, min=1.0) * fac[..., 0]
    return lg.cpu().numpy(), beta.cpu().numpy(), hn, hb


def cpu_observations(N, B, seed=1):
    """Observations [B, N, 6N] (fp32 values, as a torch fp64 tensor) of freshly reset envs from the NumPy oracle: the
    distribution of the GPU tests' first step."""
    from oracle import formation_oracle as O
    st = O.reset_hd(seed + 1000 * np.arange(B), N)
    obs = O.observation_hd(st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"])
    return torch.as_tensor(np.asarray(obs, dtype=np.float32).astype(np.float64))


# ---- the standalone fg_actor_categorical inputs (GPU test 2) ----
def standalone_inputs(seed=5, rows=4096):
    """(logits fp32 [rows, 5], u fp32 [rows]): normal logits of several scales, then the edge rows - all-equal logits, one
    logit at +100 against -100 (the other classes underflow), ties of two and three maxima - and u = 0 and the largest u
    (1 - 2^-24) cycled over every kind of row."""
    rng = np.random.RandomState(seed)
    lg = (rng.standard_normal((rows, 5)) * rng.choice([0.1, 1.0, 3.0, 10.0], (rows, 1))).astype(np.float32)
    lg[0::64] = 0.75                                      # all equal
    lg[1::64] = -100.0; lg[1::64, 3] = 100.0              # one class, the others underflow
    lg[2::64, 1] = lg[2::64, 4] = np.abs(lg[2::64]).max(-1) + 1.0     # a tie of two maxima (1 and 4)
    lg[3::64, 0] = lg[3::64, 2] = lg[3::64, 3] = 7.0      # a tie of three
    lg[3::64, 1] = lg[3::64, 4] = -2.0
    u = ((rng.randint(0, 1 << 24, rows)).astype(np.float64) * 2.0 ** -24).astype(np.float32)
    u[0::5] = 0.0
    u[1::5] = np.float32(1.0 - 2.0 ** -24)
    return lg, u
