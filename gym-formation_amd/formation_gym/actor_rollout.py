"""Which launch runs `env.rollout_actor(K, actor)`: the fused closed loop (`fg_rollout_hd_actor`, the actor evaluated inside
the rollout kernel) or the host-paced loop (`actor(obs); env.step(a)` in Python).

The fused kernel takes one actor shared by every agent, exactly
    torch.nn.Sequential(Linear(6N, H), ReLU(), Linear(H, H), ReLU(), Linear(H, 2) [, Tanh()])
with H in {32, 64, 128}, fp32 contiguous parameters on the env's device (a None bias counts as zero), for N in
{3, 4, 8, 9, 16, 25, 27, 32} agents of formation_hd_env with continuous actions, silent agents, no World options and no
post_step_callback.  Anything else runs host-paced: a shape or option the kernel cannot honour never runs fused.

The MAPPO trainers' actor (onpolicy's MLPBase) is the same body with LayerNorms: exactly
    Sequential([LayerNorm(6N),] Linear(6N, H), ReLU(), LayerNorm(H), Linear(H, H), ReLU(), LayerNorm(H), Linear(H, 2) [, Tanh()])
with H in FUSED_LN_HIDDEN = {32, 64}; the leading LayerNorm (feature normalisation) is optional, the two hidden ones come
together.  Each LayerNorm normalises the last axis only (normalized_shape == (width,)), with any positive finite eps and either
fp32 contiguous weight / bias on the env's device or none (a missing weight counts as 1, a missing bias as 0).  It fuses
(`fg_rollout_hd_actor_norm`) under the Linear body's rule, alone or as a GaussianActor's mean, in formation_hd_env only.
Host-paced: H = 128 with norms, a single hidden norm, a norm before the ReLU or anywhere else, a norm over more than the last
axis, norm parameters in another dtype, non-contiguous or off the device, PerAgentActor members with norms, and any LayerNorm
actor in the landmark scenarios (their `actor_fused_rule` states `fused_ln_hidden=()`: no such kernel).

A `GaussianActor(mean, log_std)` explores: it fuses (`fg_rollout_hd_actor_sample`) when its mean fuses as above and its
log_std is a contiguous fp32 [2] tensor on the env's device.

A `PerAgentActor(actors)` gives every agent its own network (MADDPG-style): it fuses (`fg_rollout_hd_actor_per_agent`)
when it holds N members that each fuse as above with one H and one tanh flag, alone or as the mean of a GaussianActor.

The landmark scenarios (basic_formation_env, formation_hd_partial_env, formation_hd_partial_range_env, formation_hd_obs_env)
fuse too (`fg_rollout_scenario_actor`), under the same rule with their own facts: the input width is the scenario's observation
width D instead of 6N, H in {32, 64}, and the shape is one of the seven the one-env-per-lane kernel is built for
(LANDMARK_FUSED_SHAPES).  H = 128 and a PerAgentActor run host-paced there.  The scenario states these facts
(`ActorRolloutMixin.actor_fused_rule`) and `MultiAgentEnv` hands them to `resolve_actor` below as keyword arguments, whose
defaults are formation_hd_env's.  `resolve_actor` answers the whole question once per call: None (host-paced) or the
FusedActor record the scenario's `bind_rollout_actor` takes."""
import collections
import math

import torch

LOG_2PI = math.log(2.0 * math.pi)

FUSED_N = (3, 4, 8, 9, 16, 25, 27, 32)
FUSED_HIDDEN = (32, 64, 128)
FUSED_LN_HIDDEN = (32, 64)             # hidden widths of the LayerNorm actor's kernels (ln_actor_kernel / ln_sample_kernel)
# the landmark scenarios: (scenario kind, agents, landmarks, obstacles, neighbours observed) -> fused; kind as _native.FG_SCN_*
LANDMARK_FUSED_SHAPES = ((1, 3, 3, 0, 2), (2, 5, 5, 0, 3), (2, 3, 5, 0, 3), (3, 4, 4, 0, 3), (3, 3, 4, 0, 2),
                         (4, 4, 4, 3, 3), (4, 3, 4, 3, 2))
LANDMARK_FUSED_HIDDEN = (32, 64)


def landmark_facts(kind, num_agents, num_landmarks, num_obstacles, num_obs, obs_dim, variant=0):
    """The keyword facts of `actor_path` / `actor_spec` for a landmark scenario whose shape has the fused actor launch - one of
    LANDMARK_FUSED_SHAPES, not the run-time-count kernel (variant 1) - else None: host-paced.  `num_obs` counts only for
    formation_hd_partial_env (kind 2); the other kinds observe all N - 1 neighbours."""
    N = int(num_agents)
    nbr = int(num_obs) if int(kind) == 2 else N - 1
    if int(variant) == 1 or (int(kind), N, int(num_landmarks), int(num_obstacles), nbr) not in LANDMARK_FUSED_SHAPES:
        return None
    return dict(in_features=int(obs_dim), fused_n=(N,), fused_hidden=LANDMARK_FUSED_HIDDEN, per_agent=False)


def _body_spec(actor, num_agents, device=None, in_features=None, fused_n=FUSED_N, fused_hidden=FUSED_HIDDEN,
               fused_ln_hidden=FUSED_LN_HIDDEN):
    """(hidden, out_tanh, [w1, b1, w2, b2, w3, b3], norms) when a fused kernel can evaluate the shared actor body `actor` for
    `num_agents` agents, else None.  The two forms, each with its own kernels and so its own hidden widths:
        Sequential(Linear(D, H), ReLU(), Linear(H, H), ReLU(), Linear(H, 2) [, Tanh()])              H in `fused_hidden`
        Sequential([LayerNorm(D),] Linear(D, H), ReLU(), LayerNorm(H), Linear(H, H), ReLU(), LayerNorm(H), Linear(H, 2)
                   [, Tanh()])                                                                       H in `fused_ln_hidden`
    `norms` is None for the first and the ActorNorms of the second, whose every LayerNorm is over its last axis alone with
    fp32 contiguous parameters on `device` or none.  `device`: the env's device (None: not checked).  The tensors are the
    actor's own parameters (b* may be None).  The scenario's facts: `in_features` the input width D (None:
    formation_hd_env's 6N), `fused_n` the agent counts and `fused_hidden` / `fused_ln_hidden` the hidden widths its kernels
    are built for (None or empty: it has no kernel for that form)."""
    nn = torch.nn
    if type(actor) is not nn.Sequential or int(num_agents) not in fused_n:
        return None
    if in_features is None:
        in_features = 6 * int(num_agents)
    mods = list(actor)
    lead = bool(mods) and type(mods[0]) is nn.LayerNorm
    rest = mods[1:] if lead else mods
    kinds = [type(m) for m in rest]
    out_tanh = kinds[-1:] == [nn.Tanh]
    if out_tanh:
        kinds.pop()
    if kinds == [nn.Linear, nn.ReLU, nn.Linear, nn.ReLU, nn.Linear] and not lead:
        spec = _linears_spec(rest[0], rest[2], rest[4], out_tanh, in_features, device, fused_hidden)
        return None if spec is None else spec + (None,)
    if kinds != [nn.Linear, nn.ReLU, nn.LayerNorm, nn.Linear, nn.ReLU, nn.LayerNorm, nn.Linear]:
        return None
    spec = _linears_spec(rest[0], rest[3], rest[6], out_tanh, in_features, device, fused_ln_hidden)
    if spec is None:
        return None
    dev = None if device is None else torch.device(device)
    n0 = _norm_triple(mods[0], rest[0].in_features, dev) if lead else None
    n1, n2 = _norm_triple(rest[2], spec[0], dev), _norm_triple(rest[5], spec[0], dev)
    if (lead and n0 is None) or n1 is None or n2 is None:
        return None
    return spec + (ActorNorms(n0, n1, n2),)


def actor_spec(actor, num_agents, device=None, **facts):
    """(hidden, out_tanh, [w1, b1, w2, b2, w3, b3]) when the fused kernel can evaluate the actor without LayerNorms `actor`
    for `num_agents` agents, else None: `_body_spec`'s answer (same arguments) for its first form.  This function never
    accepts a LayerNorm."""
    spec = _body_spec(actor, num_agents, device, **facts)
    return spec[:3] if spec is not None and spec[3] is None else None


def layernorm_spec(actor, num_agents, device=None, **facts):
    """(hidden, out_tanh, [w1, b1, w2, b2, w3, b3], ActorNorms) when the fused LayerNorm kernel can evaluate `actor` for
    `num_agents` agents, else None: `_body_spec`'s answer (same arguments) for its second form.  An actor without
    LayerNorms is `actor_spec`'s, not this function's."""
    spec = _body_spec(actor, num_agents, device, **facts)
    return spec if spec is not None and spec[3] is not None else None


def _linears_spec(l1, l2, l3, out_tanh, in_features, device, fused_hidden):
    """(hidden, out_tanh, [w1, b1, w2, b2, w3, b3]) of the three Linears of a body whose module kinds have been checked, else
    None.  `fused_hidden`: the hidden widths of that body's kernels (None or empty: none)."""
    H = l1.out_features
    if H not in tuple(fused_hidden or ()) or l1.in_features != int(in_features) or (l2.in_features, l2.out_features) != (H, H) \
            or (l3.in_features, l3.out_features) != (H, 2):
        return None
    params = [l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias]
    dev = None if device is None else torch.device(device)
    for t in params:
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous():
            return None
        if not _on_device(t, dev):
            return None
    return H, out_tanh, params


class ActorNorms(collections.namedtuple("ActorNorms", "input hidden1 hidden2")):
    """The LayerNorms of a fused LayerNorm actor (`_body_spec`): each a (weight, bias, eps) triple - the module's own
    parameter tensors, None where it has none (weight: 1, bias: 0), and its eps as a float; `input` is None when the actor has
    no leading LayerNorm."""
    __slots__ = ()


def _norm_triple(m, width, device):
    """(weight, bias, eps) of the LayerNorm `m` over a last axis of `width`, as the fused kernel can read it, else None."""
    if type(m) is not torch.nn.LayerNorm or tuple(m.normalized_shape) != (int(width),):
        return None
    eps = float(m.eps)
    if not (eps > 0.0 and math.isfinite(eps)):
        return None
    g, b = m.weight, getattr(m, "bias", None)
    for t in (g, b):
        if t is None:
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (int(width),) or not t.is_contiguous() \
                or not _on_device(t, device):
            return None
    return g, b, eps


class PerAgentActor(torch.nn.Module):
    """One actor per agent (no parameter sharing): `actors[i]` maps agent i's observation rows [..., 6N] to its actions
    [..., 2].  `forward(obs [..., N, 6N])` returns [..., N, 2] with out[..., i, :] = actors[i](obs[..., i, :]), which is
    what the host-paced loop runs and what the fused kernel computes."""

    def __init__(self, actors):
        super().__init__()
        self.actors = torch.nn.ModuleList(actors)

    def forward(self, obs):
        if obs.shape[-2] != len(self.actors):
            raise ValueError("obs has %d agents, the actor %d" % (obs.shape[-2], len(self.actors)))
        return torch.stack([a(obs[..., i, :]) for i, a in enumerate(self.actors)], dim=-2)


def per_agent_spec(actor, num_agents, device=None):
    """(hidden, out_tanh, [[w1, b1, w2, b2, w3, b3] per agent]) when the fused kernel can evaluate the PerAgentActor `actor`
    for `num_agents` agents, else None: N members, each passing actor_spec, all with the same H and tanh flag."""
    if not isinstance(actor, PerAgentActor) or len(actor.actors) != int(num_agents):
        return None
    specs = [actor_spec(a, num_agents, device) for a in actor.actors]
    if any(s is None for s in specs) or len({(s[0], s[1]) for s in specs}) != 1:
        return None
    return specs[0][0], specs[0][1], [s[2] for s in specs]


class GaussianActor(torch.nn.Module):
    """A diagonal Gaussian policy with a state-independent log-std (onpolicy's DiagGaussian): the action is
    mean(obs) + exp(log_std) * eps, eps ~ N(0, I), with no clipping and no tanh after the noise.
    `mean` maps observations [..., 6N] to [..., 2]; `log_std` is an nn.Parameter [2] (zeros when not given).
    `forward` draws eps with torch.randn_like and is meant for use outside the env: inside `env.rollout_actor` the env's
    counter stream supplies eps (`fg_actor_noise`), and the log-density of each action comes back in info['log_prob']."""

    def __init__(self, mean, log_std=None):
        super().__init__()
        self.mean = mean
        if log_std is None:
            log_std = torch.zeros(2)
        self.log_std = log_std if isinstance(log_std, torch.nn.Parameter) else torch.nn.Parameter(torch.as_tensor(log_std))

    def forward(self, obs):
        mu = self.mean(obs)
        return mu + torch.exp(self.log_std) * torch.randn_like(mu)

    def distribution(self, obs):
        """torch.distributions.Normal(mean(obs), exp(log_std)) of the per-component actions."""
        mu = self.mean(obs)
        return torch.distributions.Normal(mu, torch.exp(self.log_std).expand_as(mu))

    def log_prob(self, obs, act):
        """Log-density of `act` [..., 2] under the policy at `obs`, summed over the last axis (the PPO ratio's input);
        differentiable in the mean's parameters and in log_std."""
        z = (act - self.mean(obs)) * torch.exp(-self.log_std)
        return -0.5 * (z * z).sum(-1) - self.log_std.sum() - LOG_2PI

    def entropy(self):
        """Entropy of the action distribution (the same for every state): sum(log_std) + log(2 pi e)."""
        return self.log_std.sum() + LOG_2PI + 1.0


def _on_device(t, device):
    if device is None:
        return True
    dev = torch.device(device)
    return t.device.type == dev.type and (dev.index is None or t.device.index == dev.index)


def sample_spec(actor, num_agents, device=None, **facts):
    """(actor_spec(actor.mean, ...), log_std) when the fused kernel can sample from the GaussianActor `actor` for
    `num_agents` agents, else None: its mean fuses without LayerNorms (actor_spec; per_agent_spec for a PerAgentActor mean)
    and log_std is a contiguous fp32 [2] tensor on `device` (None: not checked).  log_std is the actor's own parameter, read
    in place by every launch.  `facts`: the scenario's facts for a shared mean, as `_body_spec` takes them."""
    if not isinstance(actor, GaussianActor):
        return None
    if isinstance(actor.mean, PerAgentActor):
        spec = per_agent_spec(actor.mean, num_agents, device)
    else:
        spec = actor_spec(actor.mean, num_agents, device, **facts)
    ls = _fused_log_std(actor, device)
    if spec is None or ls is None:
        return None
    return spec, ls


def _fused_log_std(actor, device):
    """The GaussianActor's log_std when the fused launch can read it in place (contiguous fp32 [2] on `device`), else None."""
    ls = actor.log_std
    if not torch.is_tensor(ls) or ls.dtype != torch.float32 or tuple(ls.shape) != (2,) or not ls.is_contiguous() \
            or not _on_device(ls, device):
        return None
    return ls


class FusedActor(collections.namedtuple("FusedActor", "hidden out_tanh members per_agent log_std norms", defaults=(None,))):
    """An actor as the fused launch takes it (`resolve_actor`): `hidden` the width H, `out_tanh`, `members` a list of
    [w1, b1, w2, b2, w3, b3] lists - the actor's own parameter tensors, b* may be None; one entry for a shared actor,
    N for a PerAgentActor (`per_agent`) - `log_std`, a GaussianActor's [2] parameter (None: deterministic), and `norms`, the
    ActorNorms of a LayerNorm actor (None: the actor has no LayerNorm)."""
    __slots__ = ()


def resolve_actor(actor, num_agents, device=None, fused_scenario=True, continuous=True, silent=True, world_options=False,
                  callback=False, per_agent=True, **facts):
    """The one decision `MultiAgentEnv.actor_path` / `rollout_actor` take, with what the launch needs: a FusedActor when
    `rollout_actor(K, actor)` runs fused, None when it runs host-paced.  The keyword facts describe the env: a scenario with
    the fused launch (formation_hd_env), continuous actions, silent agents, no World options (walls, accel, max_speed,
    u_noise, per-agent properties), no post_step_callback.  `per_agent`: the scenario's launch takes a PerAgentActor
    (formation_hd_env's does, the landmark scenarios' does not); `facts`: `_body_spec`'s keyword arguments (in_features,
    fused_n, fused_hidden, fused_ln_hidden), as the scenario states them.  A GaussianActor is unwrapped once, into its mean and
    its log_std; the mean - or the actor itself - is a PerAgentActor (per_agent_spec: members without LayerNorms) or a shared
    body (`_body_spec`: with LayerNorms where the scenario has such a kernel - formation_hd_env, H in {32, 64}; the landmark
    scenarios state `fused_ln_hidden=()`)."""
    if not (fused_scenario and continuous and silent) or world_options or callback:
        return None
    mean, log_std = actor, None
    if isinstance(actor, GaussianActor):
        mean, log_std = actor.mean, _fused_log_std(actor, device)
        if log_std is None:
            return None
    members_own = isinstance(mean, PerAgentActor)
    if members_own:
        spec = per_agent_spec(mean, num_agents, device) if per_agent else None
        spec = None if spec is None else spec + (None,)
    else:
        spec = _body_spec(mean, num_agents, device, **facts)
    if spec is None:
        return None
    hidden, out_tanh, weights, norms = spec
    return FusedActor(hidden, bool(out_tanh), weights if members_own else [weights], members_own, log_std, norms)


def actor_path(actor, num_agents, device=None, **facts):
    """'fused' or 'host': whether `resolve_actor` (same arguments) finds a fused launch."""
    return "host" if resolve_actor(actor, num_agents, device, **facts) is None else "fused"
