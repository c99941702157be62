"""Helpers of the BatchNorm actor tests (tests/test_actor_batchnorm_cpu.py, tests/test_gpu_actor_batchnorm.py): the actor the
tests build, its fp64 reference and bound, and the reference's mutants.  A plain module, device-agnostic: no fixtures, nothing
registered with pytest.

The actor.  `bn_actor(N, H, tanh, seed, eps, affine, small_var)` is `actor_testlib.scaled_mlp`'s body (the same bits) behind an
`InputBatchNorm(6N, eps, affine)` in eval mode with running_mean = 0.5 randn, running_var = 0.25 + 3.75 rand, gamma = 0.5 + rand,
beta = 0.5 randn; `small_var`: every seventh variance exactly 0 and the next 1e-3, so that eps decides istd there.

The bound.  The reference is `copy.deepcopy(actor).double()` on the observation each step acted on, and every action must meet
    |a32 - a64| <= TOL max(1, |a64|) max(1, s),    s = max_k |gamma_k| / sqrt(var_k + eps)   (fp64),   TOL = 1e-5.
The normalisation sees exact inputs and only rounds (a few ulp of each x'); layer 1 then sees inputs scaled by up to s, so the
plain actor's bound TOL max(1, |a64|) grows by that factor - the argument the LayerNorm tests make for rstd |gamma|.
"""
import copy

import torch

from formation_gym import InputBatchNorm, PerAgentActor
from tests.actor_fidelity import TOL
from tests.actor_testlib import ACT_SCALE, DEV

nn = torch.nn
MUTANTS = ("norm_dropped", "mean_not_subtracted", "gamma_ignored", "beta_ignored", "comm_skipped_after_norm", "eps_left_out")


def _body(D, H, tanh, seed):
    """`actor_testlib.scaled_mlp`'s modules on the CPU: the same initialisation under `seed`, times ACT_SCALE (one fp32 product
    per parameter: the same bits wherever it is taken)."""
    torch.manual_seed(seed)
    mods = [nn.Linear(D, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 2)]
    if tanh:
        mods.append(nn.Tanh())
    with torch.no_grad():
        for m in mods:
            for p in m.parameters():
                p.mul_(ACT_SCALE)
    return mods


def bn_actor(N, H, tanh=False, seed=0, eps=1e-5, affine=True, small_var=False, zero_head=False, device=None, norm=InputBatchNorm):
    """Sequential(norm(6N, eps, affine), Linear, ReLU, Linear, ReLU, Linear [, Tanh]) in eval mode (module docstring); `norm`:
    InputBatchNorm or nn.BatchNorm1d (a per-agent member's); `zero_head`: the last Linear zeroed."""
    D = 6 * N
    mods = _body(D, H, tanh, seed)
    bn = norm(D, eps=eps, affine=affine)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        bn.running_mean.copy_(0.5 * torch.randn(D, generator=g))
        bn.running_var.copy_(0.25 + 3.75 * torch.rand(D, generator=g))
        gamma, beta = 0.5 + torch.rand(D, generator=g), 0.5 * torch.randn(D, generator=g)
        if small_var:
            bn.running_var[::7] = 0.0
            bn.running_var[1::7] = 1e-3
        if affine:
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
        if zero_head:
            mods[4].weight.zero_()
            mods[4].bias.zero_()
    m = nn.Sequential(bn, *mods).eval()
    return m if device is None else m.to(device)


def per_agent_bn_actor(N, H, tanh=False, seed=0, device=None, identical=False, zero_head=False, **kw):
    """PerAgentActor of N `bn_actor` members with plain nn.BatchNorm1d norms (members see 2-D rows): distinct weights and
    statistics, eps cycling over 1e-5, 1e-3, 1e-2 and every third member without affine parameters - or, `identical`, N copies
    of one member."""
    if identical:
        members = [bn_actor(N, H, tanh, seed, device=device, norm=nn.BatchNorm1d, zero_head=zero_head, **kw) for _ in range(N)]
    else:
        members = [bn_actor(N, H, tanh, seed + 7 * i, eps=(1e-5, 1e-3, 1e-2)[i % 3], affine=i % 3 != 2, device=device,
                            norm=nn.BatchNorm1d, zero_head=zero_head, **kw) for i in range(N)]
    return PerAgentActor(members).eval()


def bn_scale(bn):
    """s = max_k |gamma_k| / sqrt(var_k + eps) of the BatchNorm `bn`, in fp64."""
    g = bn.weight.detach().double().abs() if bn.weight is not None else 1.0
    return float((g / torch.sqrt(bn.running_var.detach().double() + bn.eps)).max())


def bn_bound(actor, a64, scale=1.0):
    """The bound of the module docstring for the fp64 actions a64 of `actor` (a Sequential starting with the BatchNorm)."""
    return scale * TOL * torch.clamp(a64.abs(), min=1.0) * max(1.0, bn_scale(actor[0]))


def bn_fidelity(actor, obs_before, means, scale=1.0):
    """max err / bound of means [K,B,N,2] against `actor` in fp64 on obs_before[k]; `actor` a shared BatchNorm actor or a
    PerAgentActor of them (agent i against member i and its own s).  Asserts nothing but finiteness."""
    members = list(actor.actors) if isinstance(actor, PerAgentActor) else None
    refs = [copy.deepcopy(a).double().eval() for a in (members if members is not None else [actor])]
    worst = 0.0
    for k in range(len(means)):
        assert bool(torch.isfinite(means[k]).all()), "step %d: a non-finite action" % k
        o = obs_before[k].double()
        with torch.no_grad():
            if members is None:
                want = refs[0](o)
                bound = bn_bound(refs[0], want, scale)
            else:
                want = torch.stack([r(o[..., i, :]) for i, r in enumerate(refs)], dim=-2)
                bound = torch.stack([bn_bound(r, want[..., i, :], scale) for i, r in enumerate(refs)], dim=-2)
        worst = max(worst, float(((means[k].double() - want).abs() / bound).max()))
    return worst


def mutant(ref, name, x):
    """The fp64 reference `ref` (Sequential starting with the BatchNorm) on rows x [R, 6N] with one deliberate error."""
    r = copy.deepcopy(ref)
    bn, N = r[0], x.shape[-1] // 6
    with torch.no_grad():
        if name == "norm_dropped":
            return r[1:](x)
        if name == "comm_skipped_after_norm":
            h = bn(x)
            h[..., 2 * N:4 * N - 2] = 0
            return r[1:](h)
        if name == "mean_not_subtracted":
            bn.running_mean.zero_()
        elif name == "gamma_ignored" and bn.weight is not None:
            bn.weight.fill_(1.0)
        elif name == "beta_ignored" and bn.bias is not None:
            bn.bias.zero_()
        elif name == "eps_left_out":
            bn.running_var.sub_(bn.eps).clamp_(min=-bn.eps + 1e-30)
        return torch.nan_to_num(r(x), nan=1e9, posinf=1e9, neginf=-1e9)


def rows(N, count, seed=1):
    """Observation-like rows [count, 6N] with a zero communication block."""
    g = torch.Generator().manual_seed(seed)
    x = 0.7 * torch.randn(count, 6 * N, generator=g)
    x[:, 2 * N:4 * N - 2] = 0
    return x
