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

A `RecurrentActor(base, rnn, norm, head)` is rMAPPO's policy (onpolicy's R_Actor with use_recurrent_policy, recurrent_N = 1):
the LayerNorm body without its last Linear, one GRU step on a hidden state carried from step to step and zeroed where an episode
ended, a LayerNorm, and the action head.  It fuses (`fg_rollout_hd_actor_gru`, gru_actor_kernel / gru_sample_kernel) under the
LayerNorm actor's rule with H in FUSED_GRU_HIDDEN = {32, 64}, `rnn` an nn.GRUCell(H, H) or a single-layer unidirectional
nn.GRU(H, H) with biases, `norm` a LayerNorm(H) as above and `head` Linear(H, 2) or Sequential(Linear(H, 2), Tanh()), alone or as
a GaussianActor's mean, in formation_hd_env only.  Host-paced (the same loop in Python, with the same state handling): a base
without norms, H = 128, a multi-layer or bidirectional GRU, a missing norm after the GRU, recurrent PerAgentActor members, and
the landmark scenarios (`fused_gru_hidden=()`).

The MADDPG trainers' actor (train/maddpg-v2's MLPNetwork with norm_in) is the plain body behind a BatchNorm over its input,
one network per agent, in eval mode while acting: exactly
    Sequential(BatchNorm1d(6N), Linear(6N, H), ReLU(), Linear(H, H), ReLU(), Linear(H, 2) [, Tanh()])
with H in FUSED_BN_HIDDEN = {32, 64}.  The leading module is an nn.BatchNorm1d or an `InputBatchNorm` (the same module made to
take the env's [B, N, 6N] observations: nn.BatchNorm1d reads axis 1 of a 3-D input as its channels) in eval mode with
track_running_stats, num_features == 6N, running_mean / running_var fp32 contiguous [6N] on the env's device, a positive finite
eps and weight / bias fp32 contiguous [6N] on the device or none (affine=False: 1 and 0).  It fuses as a shared actor
(`fg_rollout_hd_actor_bn`) and as the members of a PerAgentActor (`fg_rollout_hd_actor_bn_per_agent`: every member this form
or none, each with its own statistics, eps and affine-ness), alone or as a GaussianActor's mean, in formation_hd_env only; the
statistics are read in place like the weights, and the rule is evaluated per call, so `actor.train()` / `actor.eval()` between
calls switch the path.  Host-paced: training mode (batch statistics are a function of the whole batch),
track_running_stats=False, a BatchNorm anywhere but first, in front of the LayerNorm form or in a RecurrentActor's base, H = 128,
statistics in another dtype or off the device, mixed PerAgentActor members, and the landmark scenarios
(`fused_bn_hidden=()`).

An `OUNoiseActor(actor, theta, sigma, scale, mu, clip)` is the MADDPG trainers' exploration on a deterministic actor:
    x <- x + theta * (mu - x) + sigma * eps;   a = clamp(actor(o) + scale * x, -clip, clip)
with the Ornstein-Uhlenbeck state x [B, N, 2] carried from step to step, set back to mu where a step ended an episode, and eps
the env's counter stream (a GaussianActor's draws).  It fuses (`fg_rollout_hd_actor_ou`, `fg_rollout_hd_actor_ou_per_agent`) in
formation_hd_env when its inner actor resolves to the plain or the BatchNorm form above, shared or as a PerAgentActor; the five
scalars are plain Python numbers read at every call.  Host-paced (the same loop in Python, the state stepped by the kernels' own
device function): a LayerNorm inner actor, any inner actor that would run host-paced itself, the landmark scenarios
(`fused_ou=False`) and World options.  A GaussianActor stays "no clipping".

A `CategoricalActor(logits)` is the MAPPO / rMAPPO trainers' discrete-action policy (`make_env(..., discrete_action=True)`):
`logits` maps observations to five logits, an index is sampled from Categorical(logits=...) - or, with `deterministic`, its mode
is taken - and the env turns the index into the raw action.  It fuses (`fg_rollout_hd_actor_cat`: cat_actor_kernel,
ln_cat_actor_kernel, gru_cat_actor_kernel) in formation_hd_env when the env is in one of the action modes FG_ACT_ONEHOT5
(`discrete_action_space`) or FG_ACT_INDEX (`discrete_action_input`) and `logits` is the plain form, the LayerNorm form or a
RecurrentActor as above with the head Linear(H, 5) and no Tanh, under the existing rules (silent agents, no World options, no
callback); `deterministic` is read at every launch.  Host-paced (the same loop in Python, the pick and the decode by the kernels'
own device functions, `fg_actor_uniform` + `fg_actor_categorical`): a head of any other width, a Tanh after it, PerAgentActor
members, a leading BatchNorm, H = 128 with norms, the landmark scenarios (`fused_cat=False`) and World options.  No path at all:
FG_ACT_ARGMAX (`force_discrete_action`), any other actor in a discrete action mode, a CategoricalActor on a continuous env.

A `GumbelSoftmaxActor(logits, explore=True)` is the MADDPG trainers' discrete action (maddpg-pytorch's agents on
`make_env(..., discrete_action=True)`): exploring, `gumbel_softmax(logits, hard=True)` - the one-hot of argmax(logits + g), g five
Gumbel draws per row from a counter stream of their own (`env.actor_gumbel()`) - and otherwise `onehot_from_logits(logits)`, the
lowest index of the largest logit.  The temperature does not enter (argmax softmax(y / T) = argmax y).  It is the OUNoiseActor's
discrete twin and fuses where that one does (`fg_rollout_hd_actor_gumbel`, `fg_rollout_hd_actor_gumbel_per_agent`:
gumbel_actor_kernel, bn_gumbel_actor_kernel, pa_gumbel_actor_kernel, pa_bn_gumbel_actor_kernel): in formation_hd_env in the modes
FG_ACT_ONEHOT5 and FG_ACT_INDEX when `logits` is the plain or the eval-mode BatchNorm form above, shared or every member of a
PerAgentActor, with the head Linear(H, 5) and no Tanh; `explore` is read at every launch.  Host-paced (the same loop in Python,
the draws, the pick and the decode by the kernels' own device functions, `fg_actor_gumbel` + `fg_actor_gumbel_pick`): a LayerNorm
or recurrent body, H = 128 behind a BatchNorm, a head of any other width, a Tanh after it, mixed members, the landmark scenarios
(`fused_gumbel=False`) and World options.  No path under FG_ACT_ARGMAX; ValueError on a continuous env.  Not built: the soft
(temperature) sample, epsilon-greedy onehot_from_logits, 16-bit observations out of this member's launch (they are cast).

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
FUSED_GRU_HIDDEN = (32, 64)            # hidden widths of the recurrent actor's kernels (gru_actor_kernel / gru_sample_kernel)
FUSED_BN_HIDDEN = (32, 64)             # hidden widths of the BatchNorm actor's kernels (bn_*_kernel / pa_bn_*_kernel)
# the landmark scenarios: (scenario kind, agents, landmarks, obstacles, neighbours observed) -> fused; kind as _native.FG_SCN_*
LANDMARK_FUSED_SHAPES = ((1, 3, 3, 0, 2), (2, 5, 5, 0, 3), (2, 3, 5, 0, 3), (3, 4, 4, 0, 3), (3, 3, 4, 0, 2),
                         (4, 4, 4, 3, 3), (4, 3, 4, 3, 2))
LANDMARK_FUSED_HIDDEN = (32, 64)
ACT_ONEHOT5, ACT_INDEX, ACT_ARGMAX = 1, 2, 3    # the env's discrete action modes (_native.FG_ACT_*); 0: continuous actions
CAT_ACTIONS = 5                                 # a CategoricalActor's head width: no move, and two directions per axis


def landmark_facts(kind, num_agents, num_landmarks, num_obstacles, num_obs, obs_dim, variant=0):
    """The keyword facts of `actor_path` / `actor_spec` for a landmark scenario whose shape has the fused actor launch - one of
    LANDMARK_FUSED_SHAPES, not the run-time-count kernel (variant 1) - else None: host-paced.  `num_obs` counts only for
    formation_hd_partial_env (kind 2); the other kinds observe all N - 1 neighbours."""
    N = int(num_agents)
    nbr = int(num_obs) if int(kind) == 2 else N - 1
    if int(variant) == 1 or (int(kind), N, int(num_landmarks), int(num_obstacles), nbr) not in LANDMARK_FUSED_SHAPES:
        return None
    return dict(in_features=int(obs_dim), fused_n=(N,), fused_hidden=LANDMARK_FUSED_HIDDEN, per_agent=False)


class InputBatchNorm(torch.nn.BatchNorm1d):
    """nn.BatchNorm1d over the LAST axis of an input of any rank: `forward` flattens every leading axis to [-1, D], applies
    BatchNorm1d's forward (train or eval mode, the running statistics updated as BatchNorm1d updates them) and restores the
    shape.  A shared actor's input norm on the env's [B, N, D] observations, where nn.BatchNorm1d takes axis 1 for its channels.
    Same parameter and buffer names as nn.BatchNorm1d, so a trainer's `in_fn` state dict loads into it."""

    def forward(self, input):
        if input.dim() < 1 or input.shape[-1] != self.num_features:
            raise ValueError("expected [..., %d] input (got %s)" % (self.num_features, tuple(input.shape)))
        return super().forward(input.reshape(-1, input.shape[-1])).reshape(input.shape)


class ActorInBn(collections.namedtuple("ActorInBn", "running_mean running_var weight bias eps")):
    """The eval-mode input BatchNorm of a fused BatchNorm actor (`_body_spec`): the module's own running_mean / running_var
    buffers and weight / bias parameters (None with affine=False: 1 and 0), read in place by every launch, and its eps as a
    float."""
    __slots__ = ()


def _param_ok(t, shape, device):
    """Whether the fused kernels can read the tensor `t` in place: fp32, contiguous, of `shape` (None: the module that owns it
    guarantees the shape) and on `device` (None: not checked)."""
    return torch.is_tensor(t) and t.dtype == torch.float32 and (shape is None or tuple(t.shape) == tuple(shape)) \
        and t.is_contiguous() and _on_device(t, device)


def _in_bn(m, width, device):
    """The ActorInBn of the leading module `m` over `width` features as the fused kernel can read it, else None: an
    nn.BatchNorm1d or InputBatchNorm in eval mode that tracks running statistics."""
    if type(m) not in (torch.nn.BatchNorm1d, InputBatchNorm) or m.training or not m.track_running_stats \
            or int(m.num_features) != int(width):
        return None
    eps = float(m.eps)
    if not (eps > 0.0 and math.isfinite(eps)):
        return None
    for t, required in ((m.running_mean, True), (m.running_var, True), (m.weight, False), (m.bias, False)):
        if (t is not None or required) and not _param_ok(t, (int(width),), device):
            return None
    return ActorInBn(m.running_mean, m.running_var, m.weight, m.bias, eps)


def _body_spec(actor, num_agents, device=None, in_features=None, fused_n=FUSED_N, fused_hidden=FUSED_HIDDEN,
               fused_ln_hidden=FUSED_LN_HIDDEN, fused_gru_hidden=FUSED_GRU_HIDDEN, fused_bn_hidden=FUSED_BN_HIDDEN,
               fused_ou=True, fused_cat=True, fused_gumbel=True, head_width=2, head_bn=False):
    """The FusedActor fields hidden, out_tanh, members = [[w1, b1, w2, b2, w3, b3]] and the form's own (below) when a fused kernel
    can evaluate the shared actor body `actor` for `num_agents` agents, else None.  The three forms, each with its own kernels
    and so its own hidden widths:
        Sequential(Linear(D, H), ReLU(), Linear(H, H), ReLU(), Linear(H, 2) [, Tanh()])              H in `fused_hidden`
        Sequential([LayerNorm(D),] Linear(D, H), ReLU(), LayerNorm(H), Linear(H, H), ReLU(), LayerNorm(H), Linear(H, 2)
                   [, Tanh()])                                                                       H in `fused_ln_hidden`
        Sequential(BatchNorm1d(D), Linear(D, H), ReLU(), Linear(H, H), ReLU(), Linear(H, 2) [, Tanh()])  H in `fused_bn_hidden`
    The first adds no field, the second `norms` - its ActorNorms, every LayerNorm over its last axis alone with fp32 contiguous
    parameters on `device` or none - and the third `in_bn`, its ActorInBn (`_in_bn`: eval mode, running statistics).
    `device`: the env's device (None: not checked).  The tensors are the
    actor's own parameters (b* may be None).  The scenario's facts: `in_features` the input width D (None:
    formation_hd_env's 6N), `fused_n` the agent counts and `fused_hidden` / `fused_ln_hidden` the hidden widths its kernels
    are built for (None or empty: it has no kernel for that form); `fused_gru_hidden` is `_recurrent_spec`'s fact and
    `fused_ou` / `fused_cat` / `fused_gumbel` (whether the scenario's launch has OU / categorical / Gumbel members)
    `resolve_actor`'s, none read here.
    `head_width`: the last Linear's outputs - 2, or CAT_ACTIONS for a CategoricalActor's or a GumbelSoftmaxActor's logits, which
    take no Tanh and - unless `head_bn`, the Gumbel member's fact: its families include the BatchNorm ones - no leading
    BatchNorm."""
    if type(actor) is not torch.nn.Sequential:
        return None
    return _modules_spec(list(actor), num_agents, device, in_features, fused_n, fused_hidden, fused_ln_hidden, fused_bn_hidden,
                         head_width, head_bn)


def _modules_spec(mods, num_agents, device, in_features, fused_n, fused_hidden, fused_ln_hidden, fused_bn_hidden=(), head_width=2,
                  head_bn=False):
    """`_body_spec` of the body whose modules, in order, are `mods`."""
    nn = torch.nn
    if int(num_agents) not in fused_n:
        return None
    if head_width != 2 and (not mods or type(mods[-1]) is nn.Tanh
                            or (not head_bn and type(mods[0]) in (nn.BatchNorm1d, InputBatchNorm))):
        return None                                        # logits: no Tanh after the head; a BatchNorm family member: `head_bn`
    if in_features is None:
        in_features = 6 * int(num_agents)
    if mods and type(mods[0]) in (nn.BatchNorm1d, InputBatchNorm):     # in front of the plain form only
        kinds = [type(m) for m in mods[1:]]
        out_tanh = kinds[-1:] == [nn.Tanh]
        if kinds[:5] != [nn.Linear, nn.ReLU, nn.Linear, nn.ReLU, nn.Linear] or len(kinds) != 5 + out_tanh:
            return None
        fields = _linears_spec(mods[1], mods[3], mods[5], out_tanh, in_features, device, fused_bn_hidden, head_width)
        bn = None if fields is None else _in_bn(mods[0], in_features, device)
        return None if bn is None else dict(fields, in_bn=bn)
    lead = bool(mods) and type(mods[0]) is nn.LayerNorm
    rest = mods[1:] if lead else mods
    kinds = [type(m) for m in rest]
    out_tanh = kinds[-1:] == [nn.Tanh]
    if out_tanh:
        kinds.pop()
    if kinds == [nn.Linear, nn.ReLU, nn.Linear, nn.ReLU, nn.Linear] and not lead:
        return _linears_spec(rest[0], rest[2], rest[4], out_tanh, in_features, device, fused_hidden, head_width)
    if kinds != [nn.Linear, nn.ReLU, nn.LayerNorm, nn.Linear, nn.ReLU, nn.LayerNorm, nn.Linear]:
        return None
    fields = _linears_spec(rest[0], rest[3], rest[6], out_tanh, in_features, device, fused_ln_hidden, head_width)
    if fields is None:
        return None
    H = fields["hidden"]
    n0 = _norm_triple(mods[0], rest[0].in_features, device) if lead else None
    n1, n2 = _norm_triple(rest[2], H, device), _norm_triple(rest[5], H, device)
    if (lead and n0 is None) or n1 is None or n2 is None:
        return None
    return dict(fields, norms=ActorNorms(n0, n1, n2))


def actor_spec(actor, num_agents, device=None, **facts):
    """(hidden, out_tanh, [w1, b1, w2, b2, w3, b3]) when the fused kernel can evaluate the actor without LayerNorms `actor`
    for `num_agents` agents, else None: `_body_spec`'s answer (same arguments) for its first form.  This function never
    accepts a LayerNorm."""
    f = _body_spec(actor, num_agents, device, **facts)
    return _shared_triple(f) if f is not None and len(f) == 3 else None


def layernorm_spec(actor, num_agents, device=None, **facts):
    """(hidden, out_tanh, [w1, b1, w2, b2, w3, b3], ActorNorms) when the fused LayerNorm kernel can evaluate `actor` for
    `num_agents` agents, else None: `_body_spec`'s answer (same arguments) for its second form.  An actor without
    LayerNorms is `actor_spec`'s, not this function's."""
    f = _body_spec(actor, num_agents, device, **facts)
    return _shared_triple(f) + (f["norms"],) if f is not None and "norms" in f else None


def batchnorm_spec(actor, num_agents, device=None, **facts):
    """(hidden, out_tanh, [w1, b1, w2, b2, w3, b3], ActorInBn) when the fused BatchNorm kernel can evaluate `actor` for
    `num_agents` agents, else None: `_body_spec`'s answer (same arguments) for its third form."""
    f = _body_spec(actor, num_agents, device, **facts)
    return _shared_triple(f) + (f["in_bn"],) if f is not None and "in_bn" in f else None


def _shared_triple(fields):
    """(hidden, out_tanh, [w1, b1, w2, b2, w3, b3]) of a shared body's FusedActor fields: what the public spec functions start
    with."""
    return fields["hidden"], fields["out_tanh"], fields["members"][0]


def _linears_spec(l1, l2, l3, out_tanh, in_features, device, fused_hidden, head_width=2):
    """The FusedActor fields hidden, out_tanh and members = [[w1, b1, w2, b2, w3, b3]] of the three Linears of a body whose
    module kinds have been checked, else None.  `fused_hidden`: the hidden widths of that body's kernels (None or empty:
    none).  `head_width`: the outputs of the last Linear - 2 for every member but the categorical one, whose CAT_ACTIONS logits
    take no Tanh."""
    H = l1.out_features
    if H not in tuple(fused_hidden or ()) or l1.in_features != int(in_features) or (l2.in_features, l2.out_features) != (H, H) \
            or (l3.in_features, l3.out_features) != (H, int(head_width)) or (head_width != 2 and out_tanh):
        return None
    params = [l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias]
    if not all(t is None or _param_ok(t, None, device) for t in params):
        return None
    return dict(hidden=H, out_tanh=bool(out_tanh), members=[params])


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
    if not all(t is None or _param_ok(t, (int(width),), device) for t in (g, b)):
        return None
    return g, b, eps


class RecurrentActor(torch.nn.Module):
    """rMAPPO's recurrent policy (onpolicy's R_Actor with use_recurrent_policy): `forward(obs [..., D], h [..., H])` returns
    (action [..., 2], h' [..., H]) with
        x = base(obs);  h' = GRU(x, h);  action = head(norm(h'))
    one step of torch.nn.GRUCell (gate order r | z | n): r = sigmoid(W_ir x + b_ir + W_hr h + b_hr), z likewise,
    n = tanh(W_in x + b_in + r * (W_hn h + b_hn)), h' = (1 - z) * n + z * h.  The state carried on is h', before the norm
    (as onpolicy's RNNLayer does).  `rnn`: an nn.GRUCell(H, H) or a single-layer unidirectional nn.GRU(H, H) - one parameter
    naming (weight_ih[_l0] ...) and one function (`torch.gru_cell`) for both, so the two give the same bits; any other nn.GRU
    is called as a module on a one-step sequence, its state [..., num_layers * directions * H] (layer-major).  `norm`:
    nn.LayerNorm(H), or None for none.  `head`: nn.Linear(H, 2) or Sequential(Linear(H, 2), Tanh()).
    `env.rollout_actor(K, actor, rnn_state=h)` runs the loop with it, zeroing h where a step ended an episode."""

    def __init__(self, base, rnn, norm, head):
        super().__init__()
        self.base, self.rnn, self.norm, self.head = base, rnn, norm, head

    def gru_parameters(self):
        """(weight_ih, weight_hh, bias_ih, bias_hh) of a GRUCell or of layer 0 of a GRU (a missing bias: None); None for
        any other module."""
        rnn = self.rnn
        if not isinstance(rnn, (torch.nn.GRUCell, torch.nn.GRU)):
            return None
        sfx = "" if isinstance(rnn, torch.nn.GRUCell) else "_l0"
        return tuple(getattr(rnn, name + sfx, None) for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))

    def _one_cell(self):
        rnn = self.rnn
        return isinstance(rnn, torch.nn.GRUCell) or (isinstance(rnn, torch.nn.GRU) and rnn.num_layers == 1
                                                     and not rnn.bidirectional and getattr(rnn, "proj_size", 0) == 0)

    @property
    def state_size(self):
        rnn = self.rnn
        if self._one_cell():
            return int(rnn.hidden_size)
        return int(rnn.num_layers) * (2 if rnn.bidirectional else 1) * int(rnn.hidden_size)

    def initial_state(self, *batch_shape):
        """Zeros [*batch_shape, H] on the parameters' device: the state of a fresh episode."""
        p = next(self.rnn.parameters())
        return torch.zeros(tuple(batch_shape) + (self.state_size,), dtype=p.dtype, device=p.device)

    def forward(self, obs, h):
        x = self.base(obs)
        lead = x.shape[:-1]
        x2 = x.reshape(-1, x.shape[-1])
        if self._one_cell():
            h_new = torch.gru_cell(x2, h.reshape(-1, h.shape[-1]), *self.gru_parameters())
            y = h_new
        else:
            rnn = self.rnn
            layers = self.state_size // int(rnn.hidden_size)
            h0 = h.reshape(-1, layers, int(rnn.hidden_size)).transpose(0, 1).contiguous()
            out, hn = rnn(x2.unsqueeze(1) if rnn.batch_first else x2.unsqueeze(0), h0)
            y = out.squeeze(1) if rnn.batch_first else out.squeeze(0)
            h_new = hn.transpose(0, 1).reshape(-1, self.state_size)
        y = y.reshape(lead + (y.shape[-1],))
        if self.norm is not None:
            y = self.norm(y)
        return self.head(y), h_new.reshape(lead + (h_new.shape[-1],))


class ActorGru(collections.namedtuple("ActorGru", "w_ih w_hh b_ih b_hh norm")):
    """The recurrent layer of a fused RecurrentActor (`_recurrent_spec`): the GRU's own parameter tensors ([3H, H], [3H, H],
    [3H], [3H]) and `norm`, the (weight, bias, eps) triple of the LayerNorm after it (`_norm_triple`)."""
    __slots__ = ()


def _recurrent_spec(actor, num_agents, device=None, in_features=None, fused_n=FUSED_N, fused_hidden=FUSED_HIDDEN,
                    fused_ln_hidden=FUSED_LN_HIDDEN, fused_gru_hidden=FUSED_GRU_HIDDEN, fused_bn_hidden=FUSED_BN_HIDDEN,
                    fused_ou=True, fused_cat=True, fused_gumbel=True, head_width=2):
    """The FusedActor fields of `_body_spec`'s LayerNorm form and `gru`, the ActorGru, when the fused recurrent kernel can evaluate
    the RecurrentActor `actor` for `num_agents` agents, else None.  Its base with its head - w3, b3 - must be the LayerNorm form
    of `_body_spec` (same arguments) with H in `fused_gru_hidden` (None or empty: the scenario has no such kernel); its GRU
    one layer, one direction, input_size == hidden_size == H, with biases; the norm after it `_norm_triple`'s; every
    parameter fp32, contiguous and on `device`.  `fused_bn_hidden` is `_body_spec`'s fact, not read here: a base that starts
    with a BatchNorm has no recurrent kernel; nor are `fused_ou`, `fused_cat` and `fused_gumbel`, `resolve_actor`'s facts.  `head_width`: the
    head's outputs, from the member - 2, or CAT_ACTIONS for a CategoricalActor's logits (a bare Linear, no Tanh)."""
    nn = torch.nn
    if type(actor) is not RecurrentActor or type(actor.base) is not nn.Sequential:
        return None
    head = actor.head
    if type(head) is nn.Linear:
        head_mods = [head]
    elif type(head) is nn.Sequential and [type(m) for m in head] == [nn.Linear, nn.Tanh]:
        head_mods = list(head)
    else:
        return None
    fields = _modules_spec(list(actor.base) + head_mods, num_agents, device, in_features, fused_n, (), fused_gru_hidden, (),
                           head_width)
    if fields is None or "norms" not in fields:
        return None
    H = fields["hidden"]
    rnn = actor.rnn
    if type(rnn) not in (nn.GRUCell, nn.GRU) or not actor._one_cell() or (rnn.input_size, rnn.hidden_size) != (H, H):
        return None
    params = actor.gru_parameters()
    if not all(_param_ok(t, shape, device) for t, shape in zip(params, ((3 * H, H), (3 * H, H), (3 * H,), (3 * H,)))):
        return None
    norm = _norm_triple(actor.norm, H, device)
    if norm is None:
        return None
    return dict(fields, gru=ActorGru(*params, norm))


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


def per_agent_spec(actor, num_agents, device=None, head_width=2):
    """(hidden, out_tanh, [[w1, b1, w2, b2, w3, b3] per agent]) when the fused kernel can evaluate the PerAgentActor `actor`
    for `num_agents` agents, else None: N members, each passing actor_spec, all with the same H and tanh flag.  `head_width`:
    every member's last Linear's outputs, as `_linears_spec` takes it (CAT_ACTIONS for a GumbelSoftmaxActor's logits)."""
    if not isinstance(actor, PerAgentActor) or len(actor.actors) != int(num_agents):
        return None
    specs = [actor_spec(a, num_agents, device, head_width=head_width) for a in actor.actors]
    if any(s is None for s in specs) or len({(s[0], s[1]) for s in specs}) != 1:
        return None
    return specs[0][0], specs[0][1], [s[2] for s in specs]


def per_agent_bn_spec(actor, num_agents, device=None, head_width=2):
    """(hidden, out_tanh, [[w1, b1, w2, b2, w3, b3] per agent], [ActorInBn per agent]) when the fused kernel can evaluate the
    PerAgentActor `actor` for `num_agents` agents with every member behind its own eval-mode input BatchNorm, else None: N
    members, each passing batchnorm_spec (nn.BatchNorm1d is fine here: members see 2-D rows), all with the same H and tanh
    flag; statistics, eps and affine-ness are each member's own.  Members of which only some have the BatchNorm: None.
    `head_width` as in `per_agent_spec`."""
    if not isinstance(actor, PerAgentActor) or len(actor.actors) != int(num_agents):
        return None
    specs = [batchnorm_spec(a, num_agents, device, head_width=head_width, head_bn=head_width != 2) for a in actor.actors]
    if any(s is None for s in specs) or len({(s[0], s[1]) for s in specs}) != 1:
        return None
    return specs[0][0], specs[0][1], [s[2] for s in specs], [s[3] for s in specs]


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

    def _mean(self, obs, rnn_state):
        """mean(obs), or for a RecurrentActor mean with its state the action part of mean(obs, rnn_state)."""
        return self.mean(obs) if rnn_state is None else self.mean(obs, rnn_state)[0]

    def forward(self, obs, rnn_state=None):
        """The sampled action; with `rnn_state` (a RecurrentActor mean's hidden state) the pair (action, new state)."""
        if rnn_state is None:
            mu = self.mean(obs)
            return mu + torch.exp(self.log_std) * torch.randn_like(mu)
        mu, h = self.mean(obs, rnn_state)
        return mu + torch.exp(self.log_std) * torch.randn_like(mu), h

    def distribution(self, obs, rnn_state=None):
        """torch.distributions.Normal(mean(obs), exp(log_std)) of the per-component actions (`rnn_state`: a recurrent mean's
        hidden state)."""
        mu = self._mean(obs, rnn_state)
        return torch.distributions.Normal(mu, torch.exp(self.log_std).expand_as(mu))

    def log_prob(self, obs, act, rnn_state=None):
        """Log-density of `act` [..., 2] under the policy at `obs` (`rnn_state`: a recurrent mean's hidden state), summed over
        the last axis (the PPO ratio's input); differentiable in the mean's parameters and in log_std."""
        z = (act - self._mean(obs, rnn_state)) * torch.exp(-self.log_std)
        return -0.5 * (z * z).sum(-1) - self.log_std.sum() - LOG_2PI

    def entropy(self):
        """Entropy of the action distribution (the same for every state): sum(log_std) + log(2 pi e)."""
        return self.log_std.sum() + LOG_2PI + 1.0


class CategoricalActor(torch.nn.Module):
    """The MAPPO / rMAPPO trainers' discrete-action policy (onpolicy's ACTLayer over a Discrete(5) space): `logits` maps
    observations [..., D] to five logits [..., 5] - the plain or LayerNorm Sequential ending in Linear(H, 5), or a RecurrentActor
    whose head is Linear(H, 5) - and the action is an index 0 .. 4 drawn from Categorical(logits=...): 0 no move, 1 .. 4 the two
    directions of each axis, as the env's action mode reads them.  `deterministic` (read at every call): the mode of the
    distribution - the lowest index of the largest logit - instead of a sample (onpolicy's `deterministic=True`).
    `forward` samples with torch and is meant for use outside the env: inside `env.rollout_actor` the env's counter stream
    supplies the uniform draw (`env.actor_uniform()`), the indices come back in info['actions'] and their log-probabilities in
    info['log_prob'].  `distribution`, `log_prob` and `entropy` are differentiable in the parameters: what a PPO update calls."""

    def __init__(self, logits, deterministic=False):
        super().__init__()
        self.logits = logits
        self.deterministic = bool(deterministic)

    def _logits(self, obs, rnn_state=None):
        """logits(obs), or for a RecurrentActor with its state the logits part of logits(obs, rnn_state)."""
        return self.logits(obs) if rnn_state is None else self.logits(obs, rnn_state)[0]

    def forward(self, obs, rnn_state=None):
        """The index [...] (int64); with `rnn_state` (a RecurrentActor's hidden state) the pair (index, new state)."""
        if rnn_state is None:
            lg, h = self.logits(obs), None
        else:
            lg, h = self.logits(obs, rnn_state)
        idx = lg.argmax(-1) if self.deterministic else torch.distributions.Categorical(logits=lg).sample()
        return idx if rnn_state is None else (idx, h)

    def distribution(self, obs, rnn_state=None):
        """torch.distributions.Categorical(logits=logits(obs)) (`rnn_state`: a recurrent body's hidden state)."""
        return torch.distributions.Categorical(logits=self._logits(obs, rnn_state))

    def log_prob(self, obs, idx, rnn_state=None):
        """Log-probability of the indices `idx` [...] under the policy at `obs`: log_softmax(logits)[idx]."""
        lsm = torch.log_softmax(self._logits(obs, rnn_state), dim=-1)
        return lsm.gather(-1, idx.to(torch.int64).unsqueeze(-1)).squeeze(-1)

    def entropy(self, obs, rnn_state=None):
        """Entropy of the action distribution at `obs` [...]: -sum_j p_j log p_j."""
        lsm = torch.log_softmax(self._logits(obs, rnn_state), dim=-1)
        return -(lsm.exp() * lsm).sum(-1)


class GumbelSoftmaxActor(torch.nn.Module):
    """The MADDPG trainers' discrete action (maddpg-pytorch's DDPGAgent.step on a discrete action space): `logits` maps
    observations [..., D] to five logits [..., 5] - one MLPNetwork per agent (a PerAgentActor) or a shared one, plain or behind
    the BatchNorm `in_fn`, ending in Linear(H, 5) - and the action is a one-hot [..., 5]:
        exploring (`explore`, read at every call):  gumbel_softmax(logits, hard=True) = one_hot(argmax(logits + g)),
                                                    g = -log(-log(U)), U uniform in (0, 1), five draws per row
        otherwise:                                  onehot_from_logits(logits) = one_hot(argmax(logits))
    with ties going to the lowest index.  There is NO temperature: the hard sample is one_hot(argmax softmax((logits + g) / T)),
    and argmax softmax(y / T) = argmax y for every T > 0, so T never changes the action; the soft sample (hard=False), which does
    depend on it, is a training-time quantity and is not built here, nor is onehot_from_logits' epsilon-greedy.
    `forward(obs, gumbel=None)` draws g with torch when none is given and is meant for use outside the env: inside
    `env.rollout_actor` the env's counter stream supplies the draws (`env.actor_gumbel()`), the indices come back in
    info['actions'] and the raw actions in info['u']; there is no log-probability (MADDPG has no use for one)."""

    def __init__(self, logits, explore=True):
        super().__init__()
        self.logits = logits
        self.explore = bool(explore)

    def forward(self, obs, gumbel=None):
        """The one-hot action [..., 5] (fp32); `gumbel` [..., 5]: the draws to explore with (None: drawn with torch)."""
        lg = self.logits(obs)
        if self.explore:
            if gumbel is None:
                u = torch.rand_like(lg).clamp_(min=torch.finfo(lg.dtype).tiny, max=1.0 - torch.finfo(lg.dtype).eps)
                gumbel = -torch.log(-torch.log(u))
            lg = lg + gumbel
        return torch.nn.functional.one_hot(lg.argmax(-1), CAT_ACTIONS).to(lg.dtype)


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
    return actor.log_std if _param_ok(actor.log_std, (2,), device) else None


class OUNoiseActor(torch.nn.Module):
    """MADDPG's exploration on a deterministic actor (train/maddpg-v2's OUNoise with its `scale`, and the clamp after it):
        x <- x + theta * (mu - x) + sigma * eps,  eps ~ N(0, I);   a = clamp(actor(obs) + scale * x, -clip, clip)
    x [..., 2] is the Ornstein-Uhlenbeck state, carried from step to step and set back to `mu` at every episode start
    (`reset_noise()`); `scale` is what the trainers anneal between episodes - the attributes are plain numbers, read anew by
    every `env.rollout_actor` call.  `clip=None`: no clamp.  With theta = 1 and mu = 0 the state has no memory, x = sigma * eps:
    i.i.d. Gaussian noise and a clip, which is maddpg-v1's exploration.
    `forward(obs, noise_state=None)` draws eps with torch.randn and returns (action, new state) - the action alone when no
    state is passed (a fresh `initial_state`) - and is meant for use outside the env: inside
    `env.rollout_actor(K, ou, noise_state=x)` the env's counter stream supplies eps (`fg_actor_noise`) and x is reset where
    a step's done flag is set.  The inner actor is deterministic: a GaussianActor, a RecurrentActor or another OUNoiseActor
    raises ValueError."""

    def __init__(self, actor, theta=0.15, sigma=0.2, scale=0.1, mu=0.0, clip=1.0):
        super().__init__()
        if isinstance(actor, (GaussianActor, RecurrentActor, OUNoiseActor)):
            raise ValueError("OUNoiseActor wraps a deterministic, stateless actor (got a %s)" % type(actor).__name__)
        self.actor = actor
        self.theta, self.sigma, self.scale, self.mu = float(theta), float(sigma), float(scale), float(mu)
        self.clip = None if clip is None else float(clip)

    def initial_state(self, *batch_shape, device=None):
        """[*batch_shape, 2] full of mu (fp32; on `device`, default the inner actor's parameters'): a fresh episode's state."""
        if device is None:
            p = next(iter(self.actor.parameters()), None) if isinstance(self.actor, torch.nn.Module) else None
            device = None if p is None else p.device
        return torch.full(tuple(batch_shape) + (2,), self.mu, dtype=torch.float32, device=device)

    def noise_step(self, noise_state, eps):
        """x + theta * (mu - x) + sigma * eps (a new tensor)."""
        return noise_state + self.theta * (self.mu - noise_state) + self.sigma * eps

    def explore(self, mean, noise_state):
        """clamp(mean + scale * x, -clip, clip): a product, a sum and the clamp, as the fused kernels evaluate it."""
        act = mean + self.scale * noise_state
        return act if self.clip is None else act.clamp(-self.clip, self.clip)

    def reset(self, noise_state, done):
        """`noise_state` with mu where `done` [...] (bool, one flag per state row or per env) is set, in place."""
        d = torch.as_tensor(done, device=noise_state.device).to(torch.bool)
        while d.dim() < noise_state.dim():
            d = d.unsqueeze(-1)
        noise_state.masked_fill_(d, self.mu)
        return noise_state

    def forward(self, obs, noise_state=None):
        mean = self.actor(obs)
        x = self.initial_state(*mean.shape[:-1], device=mean.device) if noise_state is None else noise_state
        x = self.noise_step(x, torch.randn_like(x))
        act = self.explore(mean, x)
        return act if noise_state is None else (act, x)


class FusedActor(collections.namedtuple("FusedActor", "hidden out_tanh members per_agent log_std norms gru in_bn ou cat gumbel",
                                        defaults=(None, None, None, None, None, None))):
    """An actor as the fused launch takes it (`resolve_actor`): `hidden` the width H, `out_tanh`, `members` a list of
    [w1, b1, w2, b2, w3, b3] lists - the actor's own parameter tensors, b* may be None; one entry for a shared actor,
    N for a PerAgentActor (`per_agent`) - `log_std`, a GaussianActor's [2] parameter (None: deterministic), and `norms`, the
    ActorNorms of a LayerNorm actor (None: the actor has no LayerNorm), and `gru`, the ActorGru of a RecurrentActor (None: the
    actor keeps no state), whose body is then `members[0]` with `norms` and whose head is w3, b3.  `in_bn`: the eval-mode
    input BatchNorm in front of the plain body - the (running_mean, running_var, weight, bias, eps) tuple (ActorInBn) of a
    shared actor, a list of N of them for a PerAgentActor, None without one; the tensors are the module's own.  `ou`: the
    OUNoiseActor whose exploration runs on top of the actor (None: none) - the module itself, whose scalars every launch reads.
    `cat`: the CategoricalActor whose head the members' w3 [5][H], b3 [5] are (None: a two-output head) - the module itself,
    whose `deterministic` flag every launch reads.  `gumbel`: the GumbelSoftmaxActor whose logits the members' w3 [5][H], b3 [5]
    give (None: none) - the module itself, whose `explore` flag every launch reads.
    `tensors()` and `binding_key()` are the one statement of what a launch reads by address: a binder keeps the first alive
    and a launcher cache keys on the second, so a new field is added to `_slots` and nowhere else."""
    __slots__ = ()

    def _in_bns(self):
        """The ActorInBn tuples, one per member: () without an input BatchNorm."""
        return () if self.in_bn is None else tuple(self.in_bn) if self.per_agent else (self.in_bn,)

    def _slots(self):
        """Every tensor position of the record in a fixed order - the members' weights and biases, log_std, the norms' weight and
        bias, the GRU's four tensors and its norm's two, every input BatchNorm's four - with None where the actor has none."""
        slots = [t for ws in self.members for t in ws]
        slots.append(self.log_std)
        if self.norms is not None:
            for n in self.norms:
                slots += (None, None) if n is None else n[:2]
        if self.gru is not None:
            slots += self.gru[:4] + self.gru.norm[:2]
        if self.in_bn is not None:
            for bn in self._in_bns():
                slots += bn[:4]
        return slots

    def tensors(self):
        """Every tensor the launch reads in place (`_slots` without the Nones): what a bound launcher must keep alive."""
        return tuple(t for t in self._slots() if t is not None)

    def binding_key(self):
        """What tells one binding of the record from another: the addresses of `_slots` (None kept in its place), the shape
        facts, every eps - baked into the launch's structs - and the identities of the OUNoiseActor, the CategoricalActor and the
        GumbelSoftmaxActor (the last two appended only when set), whose scalars / `deterministic` / `explore` flag are read anew
        per launch.  Equal for two resolutions of an unchanged module; a parameter re-allocated changes it."""
        eps = None                                         # the plain body has none
        if self.norms is not None or self.gru is not None or self.in_bn is not None:
            eps = (None if self.norms is None else tuple([None if n is None else n[2] for n in self.norms]),
                   None if self.gru is None else self.gru.norm[2], tuple([bn[4] for bn in self._in_bns()]))
        return (self.hidden, self.out_tanh, self.per_agent, tuple([t if t is None else t.data_ptr() for t in self._slots()]),
                eps, id(self.ou)) + (() if self.cat is None else (id(self.cat),)) \
            + (() if self.gumbel is None else (id(self.gumbel),))


def resolve_actor(actor, num_agents, device=None, fused_scenario=True, continuous=True, silent=True, world_options=False,
                  callback=False, per_agent=True, action_mode=0, **facts):
    """The one decision `MultiAgentEnv.actor_path` / `rollout_actor` take, with what the launch needs: a FusedActor when
    `rollout_actor(K, actor)` runs fused, None when it runs host-paced.  The keyword facts describe the env: a scenario with
    the fused launch (formation_hd_env), continuous actions, silent agents, no World options (walls, accel, max_speed,
    u_noise, per-agent properties), no post_step_callback.  `per_agent`: the scenario's launch takes a PerAgentActor
    (formation_hd_env's does, the landmark scenarios' does not); `facts`: `_body_spec`'s keyword arguments (in_features,
    fused_n, fused_hidden, fused_ln_hidden), as the scenario states them.  A GaussianActor is unwrapped once, into its mean and
    its log_std; the mean - or the actor itself - is a PerAgentActor (per_agent_spec: members without LayerNorms) or a shared
    body (`_body_spec`: with LayerNorms where the scenario has such a kernel - formation_hd_env, H in {32, 64}; the landmark
    scenarios state `fused_ln_hidden=()`) or a RecurrentActor (`_recurrent_spec`: formation_hd_env, H in {32, 64}; the landmark
    scenarios state `fused_gru_hidden=()`).  A leading eval-mode BatchNorm in front of the plain body - shared, or in every
    member of a PerAgentActor (per_agent_bn_spec) - fuses in formation_hd_env with H in {32, 64}; the landmark scenarios state
    `fused_bn_hidden=()`.  An OUNoiseActor is unwrapped likewise, into its inner actor and itself (`FusedActor.ou`): it fuses
    where the fact `fused_ou` holds (the scenario's launch has OU members: formation_hd_env's; the landmark scenarios state
    False) and the
    inner actor resolves to a form without LayerNorms - plain or BatchNorm, shared or per-agent.
    `action_mode`: the env's action mode as a fact - 0 continuous actions, else ACT_ONEHOT5 / ACT_INDEX / ACT_ARGMAX
    (`continuous=False` without it: some discrete mode, nothing fuses).  A CategoricalActor is unwrapped likewise, into its
    logits module and itself (`FusedActor.cat`): it fuses in the modes ACT_ONEHOT5 and ACT_INDEX where the fact `fused_cat` holds
    (formation_hd_env; the landmark scenarios state False) and its logits resolve to the plain form, the LayerNorm form or a
    RecurrentActor with a head of CAT_ACTIONS outputs and no Tanh.  A GumbelSoftmaxActor is unwrapped likewise
    (`FusedActor.gumbel`): it fuses in the same two modes where the fact `fused_gumbel` holds (formation_hd_env; the landmark
    scenarios state False) and its logits resolve to the plain or the eval-mode BatchNorm form, shared or every member of a
    PerAgentActor (where `per_agent` holds), with a head of CAT_ACTIONS outputs and no Tanh.  Every other actor fuses with
    continuous actions only."""
    if not (fused_scenario and silent) or world_options or callback:
        return None
    cat = actor if isinstance(actor, CategoricalActor) else None
    if cat is not None:
        if action_mode not in (ACT_ONEHOT5, ACT_INDEX) or not facts.get("fused_cat", True):
            return None
        logits = cat.logits
        if isinstance(logits, RecurrentActor):
            fields = _recurrent_spec(logits, num_agents, device, **dict(facts, head_width=CAT_ACTIONS))
        else:
            fields = _body_spec(logits, num_agents, device, **dict(facts, head_width=CAT_ACTIONS))
        return None if fields is None else FusedActor(per_agent=False, log_std=None, cat=cat, **fields)
    if isinstance(actor, GumbelSoftmaxActor):
        if action_mode not in (ACT_ONEHOT5, ACT_INDEX) or not facts.get("fused_gumbel", True):
            return None
        logits = actor.logits
        if isinstance(logits, PerAgentActor):
            spec, names = per_agent_spec(logits, num_agents, device, CAT_ACTIONS) if per_agent else None, ("hidden", "out_tanh", "members")
            if spec is None and per_agent and tuple(facts.get("fused_bn_hidden", FUSED_BN_HIDDEN) or ()):
                spec, names = per_agent_bn_spec(logits, num_agents, device, CAT_ACTIONS), names + ("in_bn",)
            fields = None if spec is None else dict(zip(names, spec))
        else:
            fields = _body_spec(logits, num_agents, device, **dict(facts, head_width=CAT_ACTIONS, head_bn=True))
        if fields is None or "norms" in fields:            # a LayerNorm body has no Gumbel member
            return None
        return FusedActor(per_agent=isinstance(logits, PerAgentActor), log_std=None, gumbel=actor, **fields)
    if not continuous or action_mode:
        return None
    ou = None
    if isinstance(actor, OUNoiseActor):
        if not facts.get("fused_ou", True):
            return None
        ou, actor = actor, actor.actor
    mean, log_std = actor, None
    if isinstance(actor, GaussianActor):
        mean, log_std = actor.mean, _fused_log_std(actor, device)
        if log_std is None:
            return None
    members_own = isinstance(mean, PerAgentActor)
    if members_own:
        spec, names = per_agent_spec(mean, num_agents, device) if per_agent else None, ("hidden", "out_tanh", "members")
        if spec is None and per_agent and tuple(facts.get("fused_bn_hidden", FUSED_BN_HIDDEN) or ()):
            spec, names = per_agent_bn_spec(mean, num_agents, device), names + ("in_bn",)
        fields = None if spec is None else dict(zip(names, spec))
    elif isinstance(mean, RecurrentActor):
        fields = _recurrent_spec(mean, num_agents, device, **facts)
    else:
        fields = _body_spec(mean, num_agents, device, **facts)
    if fields is None or (ou is not None and ("norms" in fields or "gru" in fields)):
        return None
    return FusedActor(per_agent=members_own, log_std=log_std, ou=ou, **fields)


def recurrent_mean(actor):
    """The RecurrentActor that `actor` is or, for a GaussianActor, has as its mean, or, for a CategoricalActor or a GumbelSoftmaxActor,
    as its logits; else None: the actor keeps no state."""
    mean = actor.mean if isinstance(actor, GaussianActor) \
        else actor.logits if isinstance(actor, (CategoricalActor, GumbelSoftmaxActor)) else actor
    return mean if isinstance(mean, RecurrentActor) else None


def actor_path(actor, num_agents, device=None, **facts):
    """'fused' or 'host': whether `resolve_actor` (same arguments) finds a fused launch."""
    return "host" if resolve_actor(actor, num_agents, device, **facts) is None else "fused"
