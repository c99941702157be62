"""GPU tests of per-agent actors: `env.rollout_actor(K, PerAgentActor([...]))`, fused (`fg_rollout_hd_actor_per_agent`,
pa_actor_kernel / pa_sample_kernel) and host-paced.  Fidelity bound: that of the shared actor (test_gpu_actor_rollout) - each
member is evaluated with the same instructions in the same k order - 1e-5 abs for tanh outputs, 1e-5 max(1, |a|) without."""
import copy

import pytest
import torch

from formation_gym import GaussianActor, PerAgentActor
from formation_gym.actor_rollout import FUSED_N
from tests.actor_testlib import (B, DEV, K, Wrap as _Wrap, clone as _clone, current_obs as _current_obs, env as _env,
                                 obs_before as _obs_before, scaled_mlp, state as _state)

pytestmark = pytest.mark.gpu

TOL = 1e-5
CASES = [(n, 64) for n in FUSED_N] + [(9, 32), (9, 128), (27, 32), (27, 128)]


def _mlp(N, H, tanh=True, seed=0):
    return scaled_mlp(6 * N, H, tanh, seed)


def _pa(N, H, tanh=True):
    """Distinct random weights per agent."""
    return PerAgentActor([_mlp(N, H, tanh, seed=100 + i) for i in range(N)])


def _check_fidelity(actor, obs_before, acts, tanh):
    ref = copy.deepcopy(actor).double()
    for k in range(len(acts)):
        with torch.no_grad():
            want = torch.stack([ref.actors[i](obs_before[k][:, i].double()) for i in range(len(ref.actors))], dim=1)
        bound = TOL if tanh else TOL * torch.clamp(want.abs(), min=1.0)
        err = (acts[k].double() - want).abs()
        assert bool((err <= bound).all()), "step %d: max err %.3g" % (k, float(err.max()))


@pytest.mark.parametrize("tanh", [True, False])
@pytest.mark.parametrize("N", [9, 27])
def test_agent_identity(N, tanh):
    # zero weights, agent i's own b3: every action of agent i is b3_i (or tanh(b3_i)) exactly, in every env and step
    env = _env(N)
    pa = _pa(N, 64, tanh)
    b3 = torch.randn(N, 2, device=DEV)
    with torch.no_grad():
        for i, m in enumerate(pa.actors):
            for p in m.parameters():
                p.zero_()
            m[4].bias.copy_(b3[i])
    assert env.actor_path(pa) == "fused"
    _, _, done, info = env.rollout_actor(K, pa)
    assert bool(done.any())
    want = torch.tanh(b3) if tanh else b3
    assert torch.equal(info["actions"], want.expand(K, B, N, 2))


@pytest.mark.parametrize("N,H", CASES)
def test_replay_and_fidelity(N, H):
    env = _env(N)
    tanh = H != 128
    pa = _pa(N, H, tanh)
    assert env.actor_path(pa) == "fused"
    snap = env._snapshot()
    obs0 = _current_obs(env)
    obs, rew, done, info = _clone(env.rollout_actor(K, pa))
    state = _state(env)
    assert bool(done.any()), "no episode boundary inside the launch"
    env._restore(snap)
    r_obs, r_rew, r_done, r_info = env.rollout(info["actions"].clone())
    assert torch.equal(obs, r_obs) and torch.equal(rew, r_rew) and torch.equal(done, r_done)
    assert torch.equal(info["individual_reward"], r_info["individual_reward"])
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)
    _check_fidelity(pa, _obs_before(obs0, obs, K), info["actions"], tanh)


@pytest.mark.parametrize("N,H", [(n, 64) for n in FUSED_N] + [(9, 128), (27, 128)])
def test_identical_members_give_the_shared_bits(N, H):
    env = _env(N)
    member = _mlp(N, H, tanh=(H != 128))
    pa = PerAgentActor([copy.deepcopy(member) for _ in range(N)])
    snap = env._snapshot()
    shared = _clone(env.rollout_actor(K, member))
    s_state = _state(env)
    env._restore(snap)
    mine = env.rollout_actor(K, pa)
    assert torch.equal(mine[3]["actions"], shared[3]["actions"])
    assert torch.equal(mine[0], shared[0]) and torch.equal(mine[1], shared[1])
    for a, b in zip(s_state, _state(env)):
        assert torch.equal(a, b)
    # the Gaussian actor: the same draws, the same bits, the same log-densities
    ls = torch.nn.Parameter(torch.tensor([-0.5, 0.3], device=DEV))
    env._restore(snap)
    g_shared = _clone(env.rollout_actor(K, GaussianActor(member, ls)))
    env._restore(snap)
    g_mine = env.rollout_actor(K, GaussianActor(pa, ls))
    assert env.actor_path(GaussianActor(pa, ls)) == "fused"
    assert torch.equal(g_mine[3]["actions"], g_shared[3]["actions"])
    assert torch.equal(g_mine[3]["log_prob"], g_shared[3]["log_prob"])
    assert torch.equal(g_mine[0], g_shared[0])


@pytest.mark.parametrize("N", [9, 27])
def test_fresh_weights_seen_by_bound_launcher(N):
    env = _env(N)
    pa = _pa(N, 64)
    f = dict(dtype=torch.float32, device=DEV)
    out = dict(obs=torch.empty((K, B, N, 6 * N), **f), reward=torch.empty((K, B, N), **f), indiv=torch.empty((K, B, N), **f),
               done=torch.zeros((K, B, N), dtype=torch.uint8, device=DEV), act=torch.empty((K, B, N, 2), **f))
    env.rollout_actor(K, pa, out=out)
    bound = dict(env._roll_launchers)
    victim = pa.actors[N // 2]                         # an SGD step on one member only
    opt = torch.optim.SGD(victim.parameters(), lr=0.05)
    victim(torch.randn(7, 6 * N, device=DEV)).square().sum().backward()
    opt.step()
    obs0 = _current_obs(env)
    obs, _, _, info = env.rollout_actor(K, pa, out=out)
    assert dict(env._roll_launchers) == bound, "the same buffers and parameters must reuse the bound launcher"
    _check_fidelity(pa, _obs_before(obs0, obs, K), info["actions"], tanh=True)


@pytest.mark.parametrize("N", [9, 27])
def test_gaussian_per_agent(N):
    env = _env(N)
    pa = _pa(N, 64)
    ls = torch.nn.Parameter(torch.tensor([-0.7, 0.2], device=DEV))
    fused = GaussianActor(pa, ls)
    assert env.actor_path(fused) == "fused"
    snap = env._snapshot()
    obs0 = _current_obs(env)
    eps0 = env.actor_noise().clone()
    f_info = _clone(env.rollout_actor(K, fused))[3]
    # eps of step 0 is env.actor_noise(): action - mean = exp(log_std) * eps to fp32 rounding
    with torch.no_grad():
        mu0 = pa(obs0)
    d = (f_info["actions"][0] - mu0) / torch.exp(ls.detach())
    assert torch.allclose(d, eps0, atol=2e-5, rtol=1e-5)
    # two launches from one snapshot: the same bits
    env._restore(snap)
    f2 = env.rollout_actor(K, fused)
    assert torch.equal(f2[3]["actions"], f_info["actions"]) and torch.equal(f2[3]["log_prob"], f_info["log_prob"])
    # the host-paced path draws the same eps: with zero means (as in test_gpu_actor_sample) both paths agree bit for bit
    zero = PerAgentActor([_mlp(N, 64, seed=100 + i) for i in range(N)])
    with torch.no_grad():
        for p in zero.parameters():
            p.zero_()
    fused = GaussianActor(zero, ls)
    host = GaussianActor(PerAgentActor([_Wrap(m) for m in zero.actors]), ls)
    assert env.actor_path(fused) == "fused" and env.actor_path(host) == "host"
    env._restore(snap)
    f_obs, f_rew, f_done, f_info = _clone(env.rollout_actor(K, fused))
    f_state = _state(env)
    env._restore(snap)
    h_obs, h_rew, h_done, h_info = env.rollout_actor(K, host)
    assert torch.equal(f_info["actions"], h_info["actions"])
    assert torch.equal(f_obs, h_obs) and torch.equal(f_rew, h_rew) and torch.equal(f_done, h_done)
    for a, b in zip(f_state, _state(env)):
        assert torch.equal(a, b)
    assert torch.allclose(f_info["log_prob"], h_info["log_prob"], rtol=1e-6, atol=0)


@pytest.mark.parametrize("N", [9, 27])
def test_unfusable_per_agent_actor_runs_host_paced(N):
    env = _env(N)
    pa = _pa(N, 64)
    pa.actors[1] = _Wrap(pa.actors[1])
    assert env.actor_path(pa) == "host"
    snap = env._snapshot()
    obs0 = _current_obs(env)
    obs, rew, done, info = env.rollout_actor(8, pa)
    with torch.no_grad():
        assert torch.equal(info["actions"][0], pa(obs0))
    env._restore(snap)
    o = obs0
    with torch.no_grad():
        for k in range(8):
            a = pa(o)
            assert torch.equal(a, info["actions"][k])
            o, r, d, _ = env.step(a)
            assert torch.equal(o, obs[k]) and torch.equal(r, rew[k])
