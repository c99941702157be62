"""What the device-RNG-counter and graph-replay tests of `rollout_actor` share (tests/test_actor_graph_cpu.py,
tests/test_gpu_actor_graph.py): the inputs, the ten cases with their actors, the draw-revealing actors and the Philox references
of the draws.  A plain module: no fixtures, nothing registered with pytest.

The setting.  A trainer captures ONE `rollout_actor` call with `env.use_device_rng_counter()` and replays it: the launch's base
offset is FgParams.rng_offset (the constant 1, frozen at capture) plus the device counter, the weights change in place between
replays, and the states (`rnn_state`, `noise_state`) are carried in device memory.  Block r = 0 is one eager call, blocks 1 .. K
are the replays; block r's step k draws at START + 3 r + k.  START = 2^32 - 8 puts the carry into the offset's high word INSIDE
replay 2 (offsets 2^32 - 2, 2^32 - 1, 2^32): it can only arrive through the counter.  world_length = 2 with auto_reset ends
episodes in every block (global steps 1, 3, 5, ...: steps [1], [0, 2], [1], [0, 2] of blocks 0 .. 3), so the reset draws run and
the OU and GRU states are reset inside every block.

The draw-revealing actors (`revealing`) make the launch's own outputs BE the draws, so that the device's draws of every replay
are held to tests/counter_rng.py, actor_cat_testlib and actor_gumbel_testlib without resting on a by-value launch being right:
  Gaussian     all weights and biases 0, log_std = 0: mean 0 and exp(0) = 1 exactly, the action is eps.
  OU           a zero inner actor, theta = 1, mu = 0, sigma = 1, scale = 1, no clip, state started at 0:
               x = fma(1, eps, fma(1, 0 - x, x)) = eps and a = 0 + 1 x = eps exactly; the state a block leaves behind is the last
               step's eps, or mu = 0 where that step ended the episode.
  categorical  head weights and bias 0: the logits are exactly 0, e_j = 1, the CDF is 1 .. 5 of 5, the index is the CDF pick of
               u at five equal probabilities and log_prob = -log 5.
  Gumbel       likewise: y_j = g_j, the index is argmax_j g_j.
The indices are compared outside the testlibs' own bands with beta = 0 (the logits are exact): `ct.exempt(margin, 0)`, ETA0 =
2^-16, and `gt.exempt(margin, 0, g)`; either band may hold at most EXEMPT_CAP = 1 % of a case's rows, which
tests/test_actor_graph_cpu.py shows the references alone to meet for every case and block.
"""
import collections

import numpy as np
import torch

from formation_gym import CategoricalActor, GaussianActor, GumbelSoftmaxActor, OUNoiseActor, PerAgentActor
from tests import actor_bn_testlib as bt
from tests import actor_cat_testlib as ct
from tests import actor_gumbel_testlib as gt
from tests import actor_ou_testlib as ot
from tests import counter_rng as R
from tests.actor_fidelity import rec_actor
from tests.actor_testlib import ACT_SCALE, DEV, scaled_mlp

nn = torch.nn

SEED, BASE = R.SEED, R.BASE
K = 3                                                  # steps per block, and replays: blocks 0 .. K
START = 2 ** 32 - 8                                    # the offset of block 0's first step
BLOCKS = K + 1
EXEMPT_CAP = gt.EXEMPT_CAP                             # 1 %: the cap of either member's band
LOG_STD = (-0.5, 0.3)
OU = dict(theta=0.15, sigma=0.3, scale=0.5, mu=0.05, clip=1.0)
DECAY = 0.9                                            # the "optimiser step" between blocks 1 and 2


def block_offsets(r):
    """The offsets of block r's K steps, in Python integers."""
    return R.launch_offsets(START + K * r, K)


Case = collections.namedtuple("Case", "num member body scenario N B H mode rnn_states_every obs_dtype")


def _case(num, member, body, N, B, H, mode=0, scenario="formation_hd_env", rnn_states_every=None, obs_dtype=None):
    return Case(num, member, body, scenario, N, B, H, mode, rnn_states_every, obs_dtype)


# the smallest shapes the members' testlibs use for a ragged last workgroup; 260 envs: two workgroups of the one-env-per-lane
# actor kernel, the second ragged
CASES = (
    _case(1, "gauss", "plain", 3, 70, 64),
    _case(2, "gauss", "gru", 9, 20, 32, rnn_states_every=2, obs_dtype=torch.bfloat16),     # the launch with the most frozen arguments
    _case(3, "ou", "bn", 27, 11, 32),
    _case(4, "ou", "pa", 9, 20, 64),
    _case(5, "cat", "ln", 27, 11, 64, ct.INDEX),
    _case(6, "cat", "gru", 3, 70, 32, ct.ONEHOT5),
    _case(7, "gumbel", "plain", 9, 20, 64, gt.ONEHOT5),
    _case(8, "gumbel", "pa_bn", 4, 70, 32, gt.INDEX),
    _case(9, "gauss", "plain", 3, 260, 32, scenario="basic_formation_env"),
    _case(10, "gauss", "plain", 4, 260, 32, scenario="formation_hd_obs_env"),
)
# the observation widths of the two landmark cases, (landmarks, obstacles, neighbours' num_obs) for the device-free rule
LANDMARK = {"basic_formation_env": (18, 3, 0, 0), "formation_hd_obs_env": (28, 4, 3, 0)}
REVEALING = (1, 3, 4, 5, 7, 9)                         # one shape per member (both OU bodies), and a landmark scenario
HOST_TWINS = (1, 4, 5, 7)                              # one case per member whose body `actor_testlib.Wrap` can hide
FROZEN = (3, 5, 7)                                     # ou.scale, cat.deterministic, gumbel.explore


def case_id(c):
    return "%d-%s-%s-%dx%d" % (c.num, c.member, c.body, c.N, c.B)


def by_num(nums):
    return [c for c in CASES if c.num in nums]


def obs_width(c):
    return 6 * c.N if c.scenario == "formation_hd_env" else LANDMARK[c.scenario][0]


# ---- the actors ----
def _mlp(D, H, tanh, seed, device, scale=ACT_SCALE):
    """`actor_testlib.scaled_mlp` on DEV; device None: its CPU twin (`actor_bn_testlib._body`: the same bits)."""
    if device is not None:
        return scaled_mlp(D, H, tanh, seed, scale)
    m = nn.Sequential(*bt._body(D, H, tanh, seed))
    if scale != ACT_SCALE:
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(scale / ACT_SCALE)
    return m


def _log_std(values, device):
    return nn.Parameter(torch.tensor(values, dtype=torch.float32, device=device))


def _inner(c, device, zero=False):
    """The OU cases' deterministic inner actor: `actor_ou_testlib.inner_actor` on DEV, the same modules on the CPU."""
    kind = {"bn": "bn", "pa": "per_agent"}[c.body]
    if device is not None:
        return ot.inner_actor(kind, c.N, c.H, False, seed=c.N, zero=zero)
    if kind == "per_agent":
        return PerAgentActor([_mlp(6 * c.N, c.H, False, c.N + 7 * i, None, 0.0 if zero else 1.5) for i in range(c.N)])
    m = bt.bn_actor(c.N, c.H, False, c.N)
    if zero:
        _zero_linears(m)
    return m


def _zero_linears(m, last_only=False):
    lins = [mod for mod in m.modules() if isinstance(mod, nn.Linear)]
    with torch.no_grad():
        for lin in (lins[-1:] if last_only else lins):
            lin.weight.zero_()
            if lin.bias is not None:
                lin.bias.zero_()
    return m


def actor(c, device=DEV):
    """The real actor of case `c` from the members' own builders, on `device` (None: the CPU, for the device-free rule)."""
    D = obs_width(c)
    if c.member == "gauss":
        mean = rec_actor(c.N, c.H, True, device=device) if c.body == "gru" else _mlp(D, c.H, c.num % 2 == 1, 0, device)
        return GaussianActor(mean, _log_std(LOG_STD, device))
    if c.member == "ou":
        return OUNoiseActor(_inner(c, device), **OU)
    if c.member == "cat":
        return ct.cat_actor(c.body, c.N, c.H, seed=ct.case_seed(c.body, c.N, c.B, c.H), device=device)
    return gt.gumbel_actor(c.body, c.N, c.H, device=device)


def revealing(c, device=DEV):
    """The draw-revealing actor of case `c`'s member at its shape (module docstring)."""
    D = obs_width(c)
    if c.member == "gauss":
        return GaussianActor(_mlp(D, c.H, False, 0, device, 0.0), _log_std((0.0, 0.0), device))
    if c.member == "ou":
        return OUNoiseActor(_inner(c, device, zero=True), theta=1.0, mu=0.0, sigma=1.0, scale=1.0, clip=None)
    if c.member == "cat":
        a = ct.cat_actor("plain", c.N, c.H, device=device)
    else:
        a = gt.gumbel_actor("plain", c.N, c.H, device=device)
    _zero_linears(a.logits, last_only=True)
    return a


def host_twin(a):
    """The same function behind `actor_testlib.Wrap`, a module the path rule does not recognise: runs host-paced."""
    from tests.actor_testlib import Wrap
    if isinstance(a, GaussianActor):
        return GaussianActor(Wrap(a.mean), a.log_std)
    if isinstance(a, OUNoiseActor):
        return OUNoiseActor(Wrap(a.actor), theta=a.theta, sigma=a.sigma, scale=a.scale, mu=a.mu, clip=a.clip)
    if isinstance(a, CategoricalActor):
        return CategoricalActor(Wrap(a.logits), a.deterministic)
    return GumbelSoftmaxActor(Wrap(a.logits), a.explore)


def decay(a, factor=DECAY):
    """An optimiser step's stand-in: every parameter (and every BatchNorm's running_mean) times `factor`, in place."""
    with torch.no_grad():
        for p in a.parameters():
            p.mul_(factor)
        for mod in a.modules():
            if isinstance(mod, nn.modules.batchnorm._BatchNorm):
                mod.running_mean.mul_(factor)


def fused_facts(c):
    """The keyword facts `actor_rollout.resolve_actor` gets from case `c`'s env, stated without a device: formation_hd_env's are
    the defaults; a landmark scenario's come from its own `actor_fused_rule` on a stand-in world."""
    import types

    from formation_gym import load_scenario
    facts = dict(continuous=not c.mode, action_mode=c.mode)
    if c.scenario != "formation_hd_env":
        _, L, M, num_obs = LANDMARK[c.scenario]
        sc = load_scenario(c.scenario)
        world = types.SimpleNamespace(agents=[None] * c.N, landmarks=[None] * (L + M))
        sc.num_agents, sc.num_landmarks, sc.num_obstacles, sc.num_obs, sc.obs_range = c.N, L, M, num_obs, 0.0
        assert sc.obs_dim(world) == obs_width(c)
        facts.update(sc.actor_fused_rule(world))
    return facts


# ---- the env, the states and one block (GPU side) ----
def env(c, offset=START):
    """Case `c`'s env, seeded and reset, auto-resetting with world_length = 2, the 64-bit seed and env_index_base of
    tests/counter_rng.py, the next launch's first step at `offset`."""
    import formation_gym
    if c.mode:
        sc = formation_gym.load_scenario(c.scenario)
        world = sc.make_world(c.N, num_envs=c.B, device=DEV)
        e = formation_gym.MultiAgentEnv(world, sc.reset_world, sc.reward, sc.observation, discrete_action=(c.mode == ct.ONEHOT5))
        e.discrete_action_input = c.mode == ct.INDEX
    else:
        e = formation_gym.make_env(c.scenario, False, c.N, num_envs=c.B, device=DEV)
    e.seed(3)
    e.reset()
    e.auto_reset = True
    e.world.world_length = 2
    e.scenario._seed = SEED                              # what `seed()` stores, without the host streams a 64-bit seed cannot key
    e.scenario.env_base = BASE
    e._rng_offset = offset - 1
    assert e._launch_rng_offset() == offset and e._action_mode() == c.mode
    return e


def states(c, a, revealed=False):
    """The state tensors case `c`'s call carries by keyword: `rnn_state` [B, N, H] (random) for a recurrent body, `noise_state`
    [B, N, 2] for an OU actor (random; zeros for the revealing one)."""
    from formation_gym.actor_rollout import recurrent_mean
    g = torch.Generator().manual_seed(7)
    st = {}
    rec = recurrent_mean(a)
    if rec is not None:
        st["rnn_state"] = (torch.rand((c.B, c.N, rec.state_size), generator=g) - 0.5).to(DEV)
    if isinstance(a, OUNoiseActor):
        st["noise_state"] = torch.zeros((c.B, c.N, 2), device=DEV) if revealed else (0.3 * torch.randn((c.B, c.N, 2), generator=g)).to(DEV)
    return st


def out_buffers(e, c, a, fused=True):
    """A caller-owned `out` with every optional tensor the member returns (act, log_prob, idx, rnn_states); False (fresh
    tensors per call) for a host-paced actor."""
    from formation_gym.actor_rollout import recurrent_mean
    if not fused:
        return False
    S = c.rnn_states_every if recurrent_mean(a) is not None else None
    want = e._rollout_shapes(K, 1, act=True, log_prob=isinstance(a, (GaussianActor, CategoricalActor)),
                             rnn_states=None if S is None else ((K + S - 1) // S, c.B, c.N, c.H),
                             idx=isinstance(a, (CategoricalActor, GumbelSoftmaxActor)))
    return {k: e._fresh_out(k, shp, c.obs_dtype) for k, shp in want.items()}


def block(e, c, a, out, st):
    """One K-step `rollout_actor` call of case `c` into `out` with the states `st`: what a trainer captures.  The states come
    back as the caller's own tensors, updated in place - a launch that worked on a copy would leave a replay nothing to carry."""
    kw = dict(st)
    if "rnn_state" in st and c.rnn_states_every is not None:
        kw["rnn_states_every"] = c.rnn_states_every
    if c.obs_dtype is not None:
        kw["obs_dtype"] = c.obs_dtype
    res = e.rollout_actor(K, a, out=out, **kw)
    for k, t in st.items():
        assert res[3][k] is t, "info[%r] is not the tensor the caller passed" % k
    return res


def env_state(e):
    """Everything a launch leaves in the simulator, by name (the tensors `MultiAgentEnv._snapshot` keeps)."""
    w, sc = e.world, e.scenario
    st = {k: getattr(w, k) for k in ("pos_x", "pos_y", "vel_x", "vel_y", "step_count", "landmark_pos", "obstacle_pos", "obstacle_vel")
          if torch.is_tensor(getattr(w, k, None))}
    st.update({k: getattr(sc, k) for k in ("ideal_shape", "ideal_vel") if torch.is_tensor(getattr(sc, k, None))})
    return st


def record(e, res, st):
    """Clones of everything a block returned and left behind, by name."""
    obs, rew, done, info = res
    rec = dict(obs=obs, reward=rew, done=done)
    rec.update({"info." + k: v for k, v in info.items()})
    rec.update({"state." + k: v for k, v in st.items()})
    rec.update({"env." + k: v for k, v in env_state(e).items()})
    return {k: v.clone() for k, v in rec.items()}


def differences(got, want):
    """The names under which two records differ (bit for bit; 16-bit and fp32 alike)."""
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    return [k for k in want if got[k].dtype != want[k].dtype or not torch.equal(got[k], want[k])]


# ---- the Philox references of a block's draws ----
def offsets_of(r, v=R.TRUE):
    """Block r's offsets as the reference variant `v` would take them: `advance` (step k at base + k) and `offset_mask`."""
    return [off & v.offset_mask for off in R.launch_offsets(START + K * r, K, v)]


def draws(member, B, N, offsets):
    """The member's draws at each of `offsets`, stacked: eps [K, B, N, 2] (Gaussian and OU), u [K, B, N], g [K, B, N, 5]."""
    one = {"gauss": lambda off: R.actor_noise(SEED, BASE, B, N, off), "ou": lambda off: R.actor_noise(SEED, BASE, B, N, off),
           "cat": lambda off: ct.uniform(SEED, BASE, B, N, off), "gumbel": lambda off: gt.gumbels(SEED, BASE, B, N, off)}[member]
    return np.stack([one(off) for off in offsets])


def reference_indices(member, d):
    """(idx, exempt) of the revealing actor's zero logits on the draws d of `draws`: the CDF pick / the argmax, and the rows
    inside the testlib's own band at beta = 0."""
    zeros = np.zeros(d.shape[:3] + (5,))
    if member == "cat":
        idx, _, margin = ct.pick(zeros, d)
        return idx, ct.exempt(margin, 0.0)
    idx, margin = gt.pick(zeros, d)
    return idx, gt.exempt(margin, 0.0, d)
