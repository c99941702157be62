"""Helpers of the OU-noise actor tests (tests/test_actor_ou_cpu.py, tests/test_gpu_actor_ou.py): the fp64 reference of the noise
state, its bound, and the actors the tests wrap.  A plain module, device-agnostic: no fixtures, nothing registered with pytest.

The state.  Per (env, agent) and component, the step that takes action k does
    x <- x + theta (mu - x) + sigma eps_k
and x <- mu after a step whose done flag is set.  `ou_reference` runs this in fp64, free from the given x0 (it never looks at
what a kernel returned), on the fp32 draws eps_k and the launch's own done flags.

The bound.  The kernels evaluate the update as fma(sigma, eps, fma(theta, mu - x, x)): three roundings per step, each at most
2^-24 of a value no larger than M = max(1, |mu|, max |x64|, sigma max |eps|) (a fourth 2^-24 M covers second-order terms and the
fp32 rounding of theta, sigma and mu themselves).  The recursion contracts errors by 1 - theta per step, so they sum to at most
    |x32 - x64| <= 4 * 2^-24 * M / theta                                                            (state_bound)
at any step; a reset to mu ends the error's history, which only helps.  The clamp is 1-Lipschitz, so an action's tolerance is the
inner actor's own bound plus `scale` times this one.
"""
import copy

import torch

from formation_gym import PerAgentActor
from tests import actor_bn_testlib as bt
from tests.actor_fidelity import TOL
from tests.actor_testlib import DEV, scaled_mlp

nn = torch.nn


def ou_reference(theta, mu, sigma, x0, eps, done):
    """The fp64 states [K, ...] each step's action used, and the final state, of the recursion of the module docstring from x0
    [..., 2] on the draws eps [K, ..., 2]; `done` [K, ...] (bool, x0's leading shape): the flags that reset to mu."""
    x = x0.double().clone()
    used = []
    for k in range(eps.shape[0]):
        x = x + theta * (mu - x) + sigma * eps[k].double()
        used.append(x.clone())
        x = torch.where(done[k].unsqueeze(-1), torch.full_like(x, mu), x)
    return torch.stack(used), x


def state_bound(theta, mu, sigma, used64, eps):
    """4 * 2^-24 * M / theta with M = max(1, |mu|, max |x64|, sigma max |eps|) over the launch (module docstring)."""
    M = max(1.0, abs(mu), float(used64.abs().max()), sigma * float(eps.abs().max()))
    return 4.0 * 2.0 ** -24 * M / theta


def inner_actor(kind, N, H, tanh, seed=0, zero=False):
    """The deterministic actor a case wraps, on DEV: 'shared' / 'per_agent' the plain MLP(s), 'bn' / 'pa_bn' the BatchNorm
    form(s); `zero`: every Linear's weights and biases 0 (the action is then the noise itself)."""
    if kind == "shared":
        m = scaled_mlp(6 * N, H, tanh, seed, scale=0.0 if zero else 1.5)
    elif kind == "per_agent":
        m = PerAgentActor([scaled_mlp(6 * N, H, tanh, seed + 7 * i, scale=0.0 if zero else 1.5) for i in range(N)])
    elif kind == "bn":
        m = bt.bn_actor(N, H, tanh, seed, device=DEV)
    elif kind == "pa_bn":
        m = bt.per_agent_bn_actor(N, H, tanh, seed, device=DEV)
    else:
        raise ValueError(kind)
    if zero and kind in ("bn", "pa_bn"):
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, nn.Linear):
                    mod.weight.zero_()
                    mod.bias.zero_()
    return m


def mean_and_bound(inner, obs):
    """(mean64, bound) of the inner actor on obs [B, N, D]: its fp64 copy's output and the family's existing actor bound -
    TOL max(1, |a64|) for the plain body, times max(1, s) behind an input BatchNorm (actor_bn_testlib.bn_bound); a
    PerAgentActor member by member."""
    def one(ref, o):
        a = ref(o)
        if isinstance(ref[0], nn.modules.batchnorm._BatchNorm):
            return a, bt.bn_bound(ref, a)
        return a, TOL * torch.clamp(a.abs(), min=1.0)
    o = obs.double()
    with torch.no_grad():
        if isinstance(inner, PerAgentActor):
            pairs = [one(copy.deepcopy(a).double().eval(), o[..., i, :]) for i, a in enumerate(inner.actors)]
            return torch.stack([p[0] for p in pairs], dim=-2), torch.stack([p[1] for p in pairs], dim=-2)
        return one(copy.deepcopy(inner).double().eval(), o)
