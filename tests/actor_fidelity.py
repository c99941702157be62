"""The fp64 references, bounds, actor builders and reference mutants the LayerNorm and recurrent actor tests share
(tests/test_gpu_actor_layernorm.py, test_gpu_actor_recurrent.py, test_gpu_actor_edges.py, test_actor_fidelity_cpu.py).  A plain
module, device-agnostic: everything works on CPU tensors as on the GPU's.  No fixtures, nothing registered with pytest.

Builders.  `ln_actor` / `rec_actor` build the MAPPO / rMAPPO actors the GPU tests launch.  With the arguments of the former
`_ln_actor` / `_rec_actor` (N, H, in_norm, tanh, seed, zero_head and one float eps) they build the same bits as those did - the
recorded figures of the GPU files rest on that, and test_actor_fidelity_cpu.py pins it.  The further knobs are independent: one
eps per norm, per-norm `elementwise_affine` / `bias`, the Linears' `bias`, a GRU weight scale of its own, GRUCell or GRU.

Bounds.  `ln_fidelity` and `rec_step_errors` carry the bounds the two GPU files derive in their docstrings:
    |a32 - a64| <= TOL max(1, |a64|) max(1, r1) max(1, r2)                          LayerNorm actor
    |h32 - h64| <= TOL max(1, r1) max(1, r2)                                        recurrent actor, state
    |a32 - a64| <= TOL max(1, |a64|) max(1, r1) max(1, r2) max(1, r3)               recurrent actor, action
r1 / r2 / r3 the rows' fp64 rstd of the two hidden norms and of the norm after the GRU.

Gate gain.  The state bound takes the error e = TOL max(1, r1) max(1, r2) of the GRU's input x through the step
    r = sigmoid(W_ir x + ..), z = sigmoid(W_iz x + ..), n = tanh(W_in x + b_in + r (W_hn h + b_hn)), h' = (1 - z) n + z h.
A gate's pre-activation moves by at most e S, S the largest row sum of |W| of its block (the infinity norm: every component of
x may be off by e), the sigmoid's slope is at most 1 / 4 and the tanh's at most 1.  The gain used here is the heuristic
    gate_gain = max(1, S_in, S_ir / 4, S_iz / 4),           S_g = max_i sum_j |W_ig[i, j]|
the largest single path's factor, clamped at 1 (the step adds rounding of its own, which TOL covers).  It is NOT a rigorous
first-order bound.  To first order dh' = (1 - z) dn + (h - n) dz, so the paths add instead of taking a maximum:
    |dh'| <= e (S_in + c S_ir / 4 + |h - n| S_iz / 4),      c = |W_hn h + b_hn|, |h - n| <= 2,
and the heuristic neglects the sum, the factor |h - n| up to 2 on the z path, and the factor c on the r path, which grows with
the GRU's weight scale (about 40 times the default in the overflow set).  In exchange it ignores that saturated gates have
slopes far below 1 / 4 and 1.  A figure above 1 against it is therefore first to be read against the full expression above
(from the fp64 reference) before it is read as a kernel's error; the measured figures are 0.036 at most.  The derivation in
test_gpu_actor_recurrent.py takes this factor as 1 ("slopes at most 1 at these weights"); at PyTorch's default initialisation
times 1.5 it is 4.9 to 6.8, and the recorded cases of that file keep their bound WITHOUT the gain - no assertion of theirs
loosens.  Cases whose GRU weights are scaled beyond that (`rec_step_errors(..., gain=True)`) multiply the state bound and the
action bound by it.  It is computed from the fp64 copies of the parameters alone, never from what a kernel returned.

Mutants.  `evaluate` is the same fp64 actor written out by hand on the parameters (`actor_params`); test_actor_fidelity_cpu.py
holds it to the module-based references (`ln_ref64` / `rec_ref64`) at 1e-12.  `mutants(params)` names the fp64 reference with
one deliberate error each and nothing else changed - the errors a kernel or its host wiring could make without the older tests
noticing.  A test that evaluates them on its own inputs and finds each at least 10 bounds away from the true reference has shown
that those inputs can see each error.
"""
import copy
import inspect
import itertools

import torch

from formation_gym import RecurrentActor
from tests.actor_testlib import ACT_SCALE

nn = torch.nn
TOL = 1e-5
NORM_BIAS_ARG = "bias" in inspect.signature(nn.LayerNorm).parameters      # torch >= 2.1: LayerNorm(..., bias=False)
NORMS = ("input", "hidden1", "hidden2", "post")                            # the order of every per-norm argument below
EDGE_EPS = (1e-3, 1e-2, 3e-2, 1e-1)                                        # distinct, ratios of 3 to 100 between any two


# ---- builders ----
def _per_norm(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v,) * 4


def _norm(width, eps, affine, bias):
    if affine and not bias:
        return nn.LayerNorm(width, eps=eps, bias=False)
    return nn.LayerNorm(width, eps=eps, elementwise_affine=bool(affine))


def _body(N, H, in_norm, eps, affine, norm_bias, linear_bias):
    D = 6 * N
    mods = [_norm(D, eps[0], affine[0], norm_bias[0])] if in_norm else []
    mods += [nn.Linear(D, H, bias=linear_bias), nn.ReLU(), _norm(H, eps[1], affine[1], norm_bias[1]),
             nn.Linear(H, H, bias=linear_bias), nn.ReLU(), _norm(H, eps[2], affine[2], norm_bias[2])]
    return mods


def _perturb_norm(mod):
    """gamma / beta away from 1 / 0, where the norm has them."""
    if mod.weight is not None:
        mod.weight.add_(0.25 * torch.randn_like(mod.weight))
    if getattr(mod, "bias", None) is not None:
        mod.bias.add_(0.2 * torch.randn_like(mod.bias))


def ln_actor(N, H, in_norm, tanh=False, seed=0, zero_head=False, eps=1e-5, affine=True, norm_bias=True, linear_bias=True,
             device=None):
    """Sequential([LayerNorm(6N),] Linear, ReLU, LayerNorm, Linear, ReLU, LayerNorm, Linear [, Tanh]): PyTorch's default
    initialisation under `seed`, the Linears times ACT_SCALE, gamma / beta away from 1 / 0.  `eps`, `affine`
    (elementwise_affine) and `norm_bias`: one value for every norm or one per norm in the order of NORMS (the fourth is the
    recurrent actor's and not read here); `linear_bias`: the three Linears'."""
    eps, affine, norm_bias = _per_norm(eps), _per_norm(affine), _per_norm(norm_bias)
    torch.manual_seed(seed)
    mods = _body(N, H, in_norm, eps, affine, norm_bias, linear_bias) + [nn.Linear(H, 2, bias=linear_bias)]
    if tanh:
        mods.append(nn.Tanh())
    m = nn.Sequential(*mods)
    with torch.no_grad():
        for mod in m:
            if isinstance(mod, nn.Linear):
                mod.weight.mul_(ACT_SCALE)
                if mod.bias is not None:
                    mod.bias.mul_(ACT_SCALE)
            elif isinstance(mod, nn.LayerNorm):
                _perturb_norm(mod)
        if zero_head:
            head = [mod for mod in m if isinstance(mod, nn.Linear)][-1]
            head.weight.zero_()
            if head.bias is not None:
                head.bias.zero_()
    return m if device is None else m.to(device)


def rec_actor(N, H, in_norm, tanh=False, seed=0, zero_head=False, eps=1e-5, affine=True, norm_bias=True, linear_bias=True,
              gru_scale=ACT_SCALE, gru=False, device=None):
    """RecurrentActor(the LayerNorm body, GRUCell(H, H), LayerNorm(H), Linear(H, 2) [- Tanh]): `ln_actor`'s initialisation and
    per-norm arguments (the fourth entry is the norm after the GRU), the GRU's parameters times `gru_scale`.  `gru`: the member
    is an nn.GRU(H, H) holding the GRUCell's tensors (copies: the same values, its own `_l0` names)."""
    eps, affine, norm_bias = _per_norm(eps), _per_norm(affine), _per_norm(norm_bias)
    torch.manual_seed(seed)
    mods = _body(N, H, in_norm, eps, affine, norm_bias, linear_bias)
    lin = nn.Linear(H, 2, bias=linear_bias)
    actor = RecurrentActor(nn.Sequential(*mods), nn.GRUCell(H, H), _norm(H, eps[3], affine[3], norm_bias[3]),
                           nn.Sequential(lin, nn.Tanh()) if tanh else lin)
    with torch.no_grad():
        for mod in actor.modules():
            if isinstance(mod, (nn.Linear, nn.GRUCell)):
                for p in mod.parameters():
                    p.mul_(gru_scale if isinstance(mod, nn.GRUCell) else ACT_SCALE)
            elif isinstance(mod, nn.LayerNorm):
                _perturb_norm(mod)
        if zero_head:
            lin.weight.zero_()
            if lin.bias is not None:
                lin.bias.zero_()
        if gru:
            cell = actor.rnn
            with torch.random.fork_rng(devices=[]):
                actor.rnn = nn.GRU(H, H)
            for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(actor.rnn, name + "_l0").copy_(getattr(cell, name))
    return actor if device is None else actor.to(device)


# ---- the module-based fp64 references and the bounds (moved from the two GPU files) ----
def ln_ref64(ref, o):
    """The fp64 actor `ref` on observations o [..., D]: (actions, r1, r2, first ReLU output), r1 / r2 the rows' rstd of the two
    hidden LayerNorms ([..., 1])."""
    x = o
    rstd, relu1 = [], None
    mods = list(ref)
    for idx, mod in enumerate(mods):
        if isinstance(mod, nn.LayerNorm) and idx > 0:
            rstd.append(1.0 / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + mod.eps))
        x = mod(x)
        if isinstance(mod, nn.ReLU) and relu1 is None:
            relu1 = x
    assert len(rstd) == 2
    return x, rstd[0], rstd[1], relu1


def ln_fidelity(actor, obs_before, means, rstd_factor=True, scale=1.0):
    """max err / bound of means [K,B,N,2] (fp64 or fp32) against the actor in fp64 on obs_before[k]; asserts nothing but
    finiteness."""
    ref = copy.deepcopy(actor).double()
    worst = 0.0
    for k in range(len(means)):
        with torch.no_grad():
            want, r1, r2, _ = ln_ref64(ref, obs_before[k].double())
        bound = scale * TOL * torch.clamp(want.abs(), min=1.0)
        if rstd_factor:
            bound = bound * torch.clamp(r1, min=1.0) * torch.clamp(r2, min=1.0)
        err = (means[k].double() - want).abs()
        assert bool(torch.isfinite(means[k]).all()), "step %d: a non-finite action" % k
        worst = max(worst, float((err / bound).max()))
    return worst


def rec_ref64(ref, o, h):
    """The fp64 actor `ref` on observations o [..., D] and states h [..., H], the GRU step by hand: (actions, new state, r1, r2,
    r3), the rows' rstd of the two hidden norms and of the norm after the GRU ([..., 1])."""
    x, rstd = o, []
    for idx, mod in enumerate(ref.base):
        if isinstance(mod, nn.LayerNorm) and idx > 0:
            rstd.append(1.0 / torch.sqrt(x.var(-1, unbiased=False, keepdim=True) + mod.eps))
        x = mod(x)
    assert len(rstd) == 2
    H = h.shape[-1]
    w_ih, w_hh, b_ih, b_hh = ref.gru_parameters()
    gi, gh = x @ w_ih.T + b_ih, h @ w_hh.T + b_hh
    r = torch.sigmoid(gi[..., :H] + gh[..., :H])
    z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    n = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    hn = (1 - z) * n + z * h
    r3 = 1.0 / torch.sqrt(hn.var(-1, unbiased=False, keepdim=True) + ref.norm.eps)
    return ref.head(ref.norm(hn)), hn, rstd[0], rstd[1], r3


def gate_gain(ref):
    """The heuristic gain max(1, S_in, S_ir / 4, S_iz / 4) of the fp64 RecurrentActor `ref`, S the largest row sum of |W| of a
    gate's block of weight_ih (module docstring, which names the terms it neglects)."""
    w_ih = ref.gru_parameters()[0].detach().double()
    H = w_ih.shape[1]
    s_r, s_z, s_n = (float(w_ih[g * H:(g + 1) * H].abs().sum(1).max()) for g in range(3))
    return max(1.0, s_n, s_r / 4.0, s_z / 4.0)


def rec_bounds(ref, a64, r1, r2, r3, scale=1.0, gain=False):
    """(action bound [..., 2], state bound [..., 1]) of the recurrent actor from its fp64 evaluation; `gain`: times gate_gain."""
    base = scale * TOL * torch.clamp(r1, min=1.0) * torch.clamp(r2, min=1.0)
    if gain:
        base = base * gate_gain(ref)
    return base * torch.clamp(a64.abs(), min=1.0) * torch.clamp(r3, min=1.0), base


def rec_step_errors(ref, obs, h_in, mean, h_out, done, scale=1.0, gain=False):
    """(action err / bound, state err / bound) maxima of one step: `mean` [B,N,2] and the masked new state `h_out` [B,N,H]
    against the fp64 actor on (obs, h_in); rows whose step ended the episode must hold exactly 0."""
    with torch.no_grad():
        a64, h64, r1, r2, r3 = rec_ref64(ref, obs.double(), h_in.double())
    a_bound, base = rec_bounds(ref, a64, r1, r2, r3, scale, gain)
    assert bool(torch.isfinite(mean).all()) and bool(torch.isfinite(h_out).all())
    a_err = float(((mean.double() - a64).abs() / a_bound).max())
    live = ~done
    assert not bool(h_out[done].any()), "a finished episode's state is not zero"
    h_err = float((((h_out.double() - h64).abs() / base)[live]).max()) if bool(live.any()) else 0.0
    assert bool((h_out[live] != 0).any(-1).all()), "a live row's state is zero"
    return a_err, h_err


# ---- the same actor by hand on its parameters, and its mutants ----
def actor_params(actor):
    """The fp64 parameters of a LayerNorm actor (Sequential) or a RecurrentActor as a dict: `norms` - NORMS' name -> (gamma or
    None, beta or None, eps), absent norms left out - `lin` - three (weight, bias or None) - `tanh`, `gru` - (w_ih, w_hh, b_ih,
    b_hh) or None."""
    rec = isinstance(actor, RecurrentActor)
    head = (list(actor.head) if isinstance(actor.head, nn.Sequential) else [actor.head]) if rec else []
    mods = (list(actor.base) if rec else list(actor)) + head
    d = lambda t: None if t is None else t.detach().double()
    lns = [m for m in mods if isinstance(m, nn.LayerNorm)]
    names = NORMS[:3] if len(lns) == 3 else NORMS[1:3]
    norms = {k: (d(m.weight), d(getattr(m, "bias", None)), float(m.eps)) for k, m in zip(names, lns)}
    if rec:
        m = actor.norm
        norms["post"] = (d(m.weight), d(getattr(m, "bias", None)), float(m.eps))
    return dict(norms=norms, lin=[(d(m.weight), d(m.bias)) for m in mods if isinstance(m, nn.Linear)],
                tanh=isinstance(mods[-1], nn.Tanh), gru=tuple(d(t) for t in actor.gru_parameters()) if rec else None)


def _comm_mask(D):
    """True at the features outside the communication block (units N .. 2N - 2 of the 3N two-float units of a row)."""
    N = D // 6
    keep = torch.ones(D, dtype=torch.bool)
    keep[2 * N:4 * N - 2] = False
    return keep


def evaluate(P, o, h=None, mutant=None):
    """The fp64 actor of `actor_params` P on observations o [..., 6N] (and states h [..., H] of a recurrent actor), written
    out: a dict with `a` (actions), `r1`, `r2`, `x` (the second hidden norm's output) and, recurrent, `h` (new state), `r3`,
    `pre_r`, `pre_z`, `pre_n` (the gates' pre-activations).  `mutant`: None, or one of `mutants(P)` - the one deliberate error."""
    kind, arg = mutant if mutant is not None else (None, None)
    norms = dict(P["norms"])
    if kind == "eps_swap":
        a, b = arg
        (ga, ba, ea), (gb, bb, eb) = norms[a], norms[b]
        norms[a], norms[b] = (ga, ba, eb), (gb, bb, ea)
    elif kind == "hidden_affine_swap":
        (g1, b1, e1), (g2, b2, e2) = norms["hidden1"], norms["hidden2"]
        norms["hidden1"], norms["hidden2"] = (g2, b2, e1), (g1, b1, e2)
    elif kind == "post_affine_ignored":
        norms["post"] = (None, None, norms["post"][2])

    def norm(x, name):
        g, b, eps = norms[name]
        xs = x[..., _comm_mask(x.shape[-1]).to(x.device)] if (kind == "input_stats_without_comm" and name == "input") else x
        mean = xs.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(xs.var(-1, unbiased=(kind == "unbiased_variance"), keepdim=True) + eps)
        y = (x - mean) * rstd
        if g is not None:
            y = y * g
        if b is not None:
            y = y + b
        return y, rstd

    lin = lambda x, wb: x @ wb[0].T + (0.0 if wb[1] is None else wb[1])
    x = o
    if "input" in norms:
        x, _ = norm(x, "input")
    x, r1 = norm(torch.relu(lin(x, P["lin"][0])), "hidden1")
    x, r2 = norm(torch.relu(lin(x, P["lin"][1])), "hidden2")
    out = dict(r1=r1, r2=r2, x=x)
    if P["gru"] is not None:
        w_ih, w_hh, b_ih, b_hh = P["gru"]
        H = h.shape[-1]
        if kind == "rz_blocks_swapped":
            perm = torch.cat((torch.arange(H, 2 * H), torch.arange(0, H), torch.arange(2 * H, 3 * H))).to(w_ih.device)
            w_ih, w_hh, b_ih, b_hh = w_ih[perm], w_hh[perm], b_ih[perm], b_hh[perm]
        gi, gh = x @ w_ih.T + b_ih, h @ w_hh.T + b_hh
        pre_r, pre_z = gi[..., :H] + gh[..., :H], gi[..., H:2 * H] + gh[..., H:2 * H]
        r, z = torch.sigmoid(pre_r), torch.sigmoid(pre_z)
        if kind == "bhn_outside_reset":
            pre_n = gi[..., 2 * H:] + r * (gh[..., 2 * H:] - b_hh[2 * H:]) + b_hh[2 * H:]
        else:
            pre_n = gi[..., 2 * H:] + r * gh[..., 2 * H:]
        n = torch.tanh(pre_n)
        hn = z * n + (1 - z) * h if kind == "z_exchanged" else (1 - z) * n + z * h
        x, r3 = norm(hn, "post")
        out.update(h=hn, r3=r3, pre_r=pre_r, pre_z=pre_z, pre_n=pre_n)
    a = lin(x, P["lin"][2])
    out["a"] = torch.tanh(a) if P["tanh"] else a
    return out


def mutants(P):
    """The (kind, argument) mutants `evaluate` knows for the parameters P: every pairwise swap of eps between the norms present,
    gamma / beta of the two hidden norms exchanged, unbiased variance in every norm, the input norm's statistics without the
    communication block (with an input norm) and, recurrent: b_hn outside the reset gate, z and 1 - z exchanged, the r and z
    row blocks of W and b exchanged, gamma3 / beta3 ignored."""
    present = [k for k in NORMS if k in P["norms"]]
    out = [("eps_swap", pair) for pair in itertools.combinations(present, 2)]
    out += [("hidden_affine_swap", None), ("unbiased_variance", None)]
    if "input" in P["norms"]:
        out.append(("input_stats_without_comm", None))
    if P["gru"] is not None:
        out += [("bhn_outside_reset", None), ("z_exchanged", None), ("rz_blocks_swapped", None), ("post_affine_ignored", None)]
    return out


def mutant_ratios(actor, o, h=None, gain=False):
    """{mutant: largest |mutant - true| / bound} on (o, h): the action's and, recurrent, the state's, against the bounds above
    built from the true fp64 reference.  No kernel involved."""
    ref = copy.deepcopy(actor).double()
    P = actor_params(ref)
    o = o.double()
    h = None if h is None else h.double()
    with torch.no_grad():
        true = evaluate(P, o, h)
        if h is None:
            a_bound = TOL * torch.clamp(true["a"].abs(), min=1.0) * torch.clamp(true["r1"], min=1.0) \
                * torch.clamp(true["r2"], min=1.0)
        else:
            a_bound, h_bound = rec_bounds(ref, true["a"], true["r1"], true["r2"], true["r3"], gain=gain)
        out = {}
        for m in mutants(P):
            got = evaluate(P, o, h, m)
            ratio = float(((got["a"] - true["a"]).abs() / a_bound).max())
            if h is not None:
                ratio = max(ratio, float(((got["h"] - true["h"]).abs() / h_bound).max()))
            out[m] = ratio
    return out


def mutant_name(m):
    return m[0] if m[1] is None else "%s(%s)" % (m[0], ",".join(m[1]))


# ---- the parameter sets of the edge tests (test_actor_fidelity_cpu.py checks on the CPU what test_gpu_actor_edges.py launches) ----
SAT_SCALE = 6.0                                        # GRU weights: a fair share of the r / z gates saturated
OVERFLOW_SCALE = 40.0                                  # ... and some pre-activations beyond 90: expf gives inf on one side, 0 on the other
EDGE_SETS = {
    "eps": dict(eps=EDGE_EPS),
    "no_affine": dict(eps=EDGE_EPS, affine=False),
    # input norm without affine, hidden 1 with gamma but no beta, hidden 2 plain, the norm after the GRU affine
    "mixed": dict(eps=EDGE_EPS, affine=(False, True, False, True), norm_bias=(True, False, True, True)),
    "mixed_no_linear_bias": dict(eps=EDGE_EPS, affine=(False, True, False, True), norm_bias=(True, False, True, True),
                                 linear_bias=False),
    "saturated": dict(eps=EDGE_EPS, gru_scale=SAT_SCALE),
    "overflow": dict(eps=EDGE_EPS, gru_scale=OVERFLOW_SCALE),
}
GAIN_SETS = ("saturated", "overflow")                  # the sets whose bounds carry gate_gain
REC_ONLY_SETS = ("saturated", "overflow")


def edge_state(shape, seed=11):
    """States uniform in (-1, 1) with, cyclically over the rows, a row of exact zeros, a row of +1, a row of -1, a row with
    every third entry one of those, and four ordinary rows."""
    g = torch.Generator().manual_seed(seed)
    h = torch.rand(shape, generator=g) * 2 - 1
    flat = h.reshape(-1, shape[-1])
    flat[0::8] = 0.0
    flat[1::8] = 1.0
    flat[2::8] = -1.0
    flat[3::8, 0::3] = 0.0
    flat[3::8, 1::6] = 1.0
    flat[3::8, 4::6] = -1.0
    return h
