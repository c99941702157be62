"""GPU tests of the BatchNorm actor rollout: `env.rollout_actor(K, actor)` with the MADDPG trainers' actor (train/maddpg-v2's
MLPNetwork with norm_in, in eval mode: BatchNorm1d - Linear - ReLU - Linear - ReLU - Linear [- Tanh]), shared
(`fg_rollout_hd_actor_bn`, bn_actor_kernel / bn_sample_kernel) and one per agent (`fg_rollout_hd_actor_bn_per_agent`,
pa_bn_actor_kernel / pa_bn_sample_kernel), deterministic and as the mean of a GaussianActor, against an fp64 reference.

Actor fidelity bound (tests/actor_bn_testlib.py).  The reference is `copy.deepcopy(actor).double()` on the observation each step
acted on; with s = max_k |gamma_k| / sqrt(var_k + eps) in fp64, every action must meet
    |a32 - a64| <= 1e-5 * max(1, |a64|) * max(1, s).
The normalisation sees exact inputs and only rounds; layer 1 then sees inputs scaled by up to s.  test_actor_batchnorm_cpu.py
holds torch's fp32 modules inside this bound and every mutant of the fp64 reference (norm dropped, mean not subtracted, gamma or
beta ignored, communication block skipped after the norm, eps left out where the variance is tiny) at least 10 bounds outside.
Each test prints its largest err / bound before it asserts <= 1.

Largest measured err / bound per case on MI355X (the whole table: profiles/actor_batchnorm.md):
test_replay_determinism_fidelity (N, H, tanh, affine): (3, 64, yes, yes) 0.015, (4, 64, no, yes) 0.010, (8, 64, yes, no) 0.009,
  (9, 64, no, no) 0.019, (16, 64, yes, yes) 0.018, (25, 64, no, yes) 0.023, (27, 64, yes, no) 0.021, (32, 64, no, no) 0.020,
  (9, 32, yes, no) 0.014, (27, 32, no, yes) 0.019
test_per_agent_members_fidelity_and_replay: N = 3 0.015, 9 0.019, 16 0.029, 27 0.027, 32 0.033
test_gaussian_mean_fidelity_replay_and_host_twin, actions - exp(log_std) eps: (9, 64) 0.027, (27, 32) 0.026, per agent (9, 64)
  0.031; host-paced twin at step 0, diff / (2 bound): 0.007, 0.009, 0.014
test_edge_statistics: (9, shared, eps 1e-2) 0.378, (32, shared, eps 1e-1) 0.001, (16, per agent, eps 1e-2) 0.342
test_statistics_read_in_place_and_mode_switches_the_path (first, copy_, load_state_dict): shared 0.021, 0.028, 0.037; per agent
  0.028, 0.069, 0.115
test_host_paced_twin_at_step_0, diff / (2 bound): (9, 64) 0.007, (27, 32) 0.007, per agent (16, 64) 0.008

Host-paced twin.  Both paths evaluate the same fp32 function on the same observation only at the first step of a launch, so the
twin is compared at step 0, within twice the bound, and over all K steps where the actions are the noise itself (zeroed head):
there the two trajectories are the same bits.
"""
import copy

import pytest
import torch

from formation_gym import GaussianActor, PerAgentActor
from formation_gym.actor_rollout import FUSED_N
from tests import actor_bn_testlib as bt
from tests.actor_testlib import (B, DEV, K, Wrap as _Wrap, clone as _clone, current_obs as _current_obs, env as _env,
                                 logp_formula as _logp_formula, noise_at as _noise_at, obs_before as _obs_before, state as _state)

pytestmark = pytest.mark.gpu
nn = torch.nn

# (N, H, tanh, affine): every N at H = 64, alternating tanh and affine, plus two shapes at H = 32
CASES = [(n, 64, i % 2 == 0, i % 4 < 2) for i, n in enumerate(FUSED_N)] + [(9, 32, True, False), (27, 32, False, True)]


def _bn_actor(*args, **kw):
    return bt.bn_actor(*args, device=DEV, **kw)


def _pa_actor(*args, **kw):
    return bt.per_agent_bn_actor(*args, device=DEV, **kw)


def _bound_at(actor, obs, scale):
    """`scale` times the bound of every action of `actor` (shared, or a PerAgentActor: member i's own) on obs [B, N, 6N]."""
    per_agent = isinstance(actor, PerAgentActor)
    refs = [copy.deepcopy(a).double() for a in (actor.actors if per_agent else [actor])]
    with torch.no_grad():
        o = obs.double()
        if not per_agent:
            return bt.bn_bound(refs[0], refs[0](o), scale)
        return torch.stack([bt.bn_bound(r, r(o[..., i, :]), scale) for i, r in enumerate(refs)], dim=-2)


def _run_checked(env, actor, tag):
    """One fused launch with the replay, determinism and fidelity checks of a deterministic actor: its (obs0, results)."""
    assert env.actor_path(actor) == "fused"
    snap = env._snapshot()
    obs0 = _current_obs(env)
    obs, rew, done, info = _clone(env.rollout_actor(K, actor))
    state = _state(env)
    assert bool(done.any()), "no episode boundary inside the launch"
    assert "log_prob" not in info
    env._restore(snap)
    r_obs, r_rew, r_done, r_info = env.rollout(info["actions"].clone())
    assert torch.equal(obs, r_obs) and torch.equal(rew, r_rew) and torch.equal(done, r_done)
    assert torch.equal(info["individual_reward"], r_info["individual_reward"])
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)
    env._restore(snap)
    obs2, rew2, _, info2 = env.rollout_actor(K, actor)
    assert torch.equal(info["actions"], info2["actions"]) and torch.equal(obs, obs2) and torch.equal(rew, rew2)
    worst = bt.bn_fidelity(actor, _obs_before(obs0, obs, K), info["actions"])
    print("BNFIDELITY %s max err/bound = %.4f" % (tag, worst))
    assert worst <= 1.0, "max err / bound = %.3g" % worst
    return obs0, (obs, rew, done, info)


@pytest.mark.parametrize("N,H,tanh,affine", CASES)
def test_replay_determinism_fidelity(N, H, tanh, affine):
    _run_checked(_env(N), _bn_actor(N, H, tanh, seed=N, affine=affine), "det N=%d H=%d tanh=%d affine=%d" % (N, H, tanh, affine))


@pytest.mark.parametrize("N", [3, 9, 16, 27, 32])
def test_per_agent_members_fidelity_and_replay(N):
    actor = _pa_actor(N, 64, tanh=N % 2 == 1, seed=N)
    assert len({float(a[0].eps) for a in actor.actors}) == 3 and any(a[0].weight is None for a in actor.actors)
    _run_checked(_env(N), actor, "per-agent N=%d" % N)


@pytest.mark.parametrize("N", [9, 27])
@pytest.mark.parametrize("gaussian", [False, True])
def test_identical_members_give_the_shared_kernels_bits(N, gaussian):
    env = _env(N)
    log_std = nn.Parameter(torch.tensor([-0.5, 0.3], device=DEV))
    shared = _bn_actor(N, 64, True, seed=5, eps=1e-3)
    members = _pa_actor(N, 64, True, seed=5, eps=1e-3, identical=True)
    one, many = (GaussianActor(shared, log_std), GaussianActor(members, log_std)) if gaussian else (shared, members)
    for a in members.actors:                                           # the same values behind a plain nn.BatchNorm1d
        assert all(torch.equal(p, q) for p, q in zip(a.state_dict().values(), shared.state_dict().values()))
    assert env.actor_path(one) == "fused" and env.actor_path(many) == "fused"
    snap = env._snapshot()
    a = _clone(env.rollout_actor(K, one))
    env._restore(snap)
    b = _clone(env.rollout_actor(K, many))
    assert torch.equal(a[3]["actions"], b[3]["actions"]) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    if gaussian:
        assert torch.equal(a[3]["log_prob"], b[3]["log_prob"])


@pytest.mark.parametrize("N,per_agent", [(9, False), (27, False), (9, True)])
def test_gaussian_exact_noise_over_two_launches_and_host_twin(N, per_agent):
    env = _env(N)
    mean = _pa_actor(N, 64, seed=2, zero_head=True) if per_agent else _bn_actor(N, 64, seed=2, zero_head=True)
    actor = GaussianActor(mean, nn.Parameter(torch.zeros(2, device=DEV)))
    host = GaussianActor(_Wrap(mean), actor.log_std)
    assert env.actor_path(actor) == "fused" and env.actor_path(host) == "host"
    seen = []
    for launch in range(2):
        want = torch.stack([_noise_at(env, k) for k in range(K)])
        snap = env._snapshot()
        obs, rew, done, info = _clone(env.rollout_actor(K, actor))
        state = _state(env)
        acts, logp = info["actions"], info["log_prob"]
        assert acts.shape == (K, B, N, 2) and logp.shape == (K, B, N)
        assert torch.equal(acts, want), "launch %d: the actions are not fg_actor_noise at each step's offset" % launch
        assert torch.allclose(logp, _logp_formula(acts, torch.zeros(2, device=DEV)), rtol=1e-6, atol=0)
        seen.append(acts)
        env._restore(snap)                                             # the host-paced twin: the same bits over all K steps
        h_obs, h_rew, h_done, h_info = env.rollout_actor(K, host)
        assert torch.equal(h_info["actions"], acts) and torch.equal(h_info["log_prob"], logp)
        assert torch.equal(h_obs, obs) and torch.equal(h_rew, rew) and torch.equal(h_done, done)
        for a, b in zip(state, _state(env)):
            assert torch.equal(a, b)
    assert not bool((seen[0] == seen[1]).all(-1).any()), "the second launch repeats draws of the first"


@pytest.mark.parametrize("N,H,per_agent", [(9, 64, False), (27, 32, False), (9, 64, True)])
def test_gaussian_mean_fidelity_replay_and_host_twin(N, H, per_agent):
    env = _env(N)
    log_std = nn.Parameter(torch.tensor([-0.5, 0.3], device=DEV))
    mean = _pa_actor(N, H, seed=4) if per_agent else _bn_actor(N, H, True, seed=4)
    actor, host = GaussianActor(mean, log_std), GaussianActor(_Wrap(mean), log_std)
    assert env.actor_path(actor) == "fused" and env.actor_path(host) == "host"
    snap = env._snapshot()
    obs0 = _current_obs(env)
    eps = torch.stack([_noise_at(env, k) for k in range(K)])
    obs, rew, done, info = _clone(env.rollout_actor(K, actor))
    state = _state(env)
    assert bool(done.any())
    env._restore(snap)
    r_obs, r_rew, r_done, _ = env.rollout(info["actions"].clone())
    assert torch.equal(obs, r_obs) and torch.equal(rew, r_rew) and torch.equal(done, r_done)
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)
    env._restore(snap)
    _, _, _, info2 = _clone(env.rollout_actor(K, actor))
    assert torch.equal(info["actions"], info2["actions"]) and torch.equal(info["log_prob"], info2["log_prob"])
    assert torch.allclose(info["log_prob"], _logp_formula(eps, log_std.detach()), rtol=1e-6, atol=0)
    mean32 = info["actions"].double() - torch.exp(log_std.detach().double()) * eps.double()
    worst = bt.bn_fidelity(mean, _obs_before(obs0, obs, K), mean32)
    print("BNFIDELITY gauss N=%d H=%d per_agent=%d max err/bound = %.4f" % (N, H, per_agent, worst))
    assert worst <= 1.0, "max err / bound = %.3g" % worst
    # the host-paced twin draws the same eps; at step 0 both act on the same observation: twice the bound
    env._restore(snap)
    _, _, _, h_info = env.rollout_actor(K, host)
    bound = _bound_at(mean, obs0, 2.0)
    diff = (h_info["actions"][0].double() - info["actions"][0].double()).abs()
    print("BNTWIN gauss N=%d H=%d per_agent=%d max diff/(2 bound) at step 0 = %.4f" % (N, H, per_agent, float((diff / bound).max())))
    assert bool((diff <= bound).all())
    assert torch.allclose(h_info["log_prob"][0], info["log_prob"][0], rtol=1e-6, atol=0)


@pytest.mark.parametrize("N,per_agent,eps", [(9, False, 1e-2), (32, False, 1e-1), (16, True, 1e-2)])
def test_edge_statistics(N, per_agent, eps):
    """Variances of exactly 0 and 1e-3 (eps decides istd), no affine parameters, and a running mean of 50 on the
    communication block: its normalised zeros are large, and layer 1 must not skip them."""
    env = _env(N)
    if per_agent:
        actor = PerAgentActor([_bn_actor(N, 64, True, seed=3 * i, eps=eps, affine=i % 2 == 0, small_var=True,
                                         norm=nn.BatchNorm1d) for i in range(N)]).eval()
        norms = [a[0] for a in actor.actors]
    else:
        actor = _bn_actor(N, 64, True, seed=1, eps=eps, affine=False, small_var=True)
        norms = [actor[0]]
    with torch.no_grad():
        for bn in norms:
            bn.running_mean[2 * N:4 * N - 2] = 50.0
    _run_checked(env, actor, "edge N=%d per_agent=%d eps=%g" % (N, per_agent, eps))


@pytest.mark.parametrize("per_agent", [False, True])
def test_statistics_read_in_place_and_mode_switches_the_path(per_agent):
    N = 9
    env = _env(N)
    actor = _pa_actor(N, 64, seed=6) if per_agent else _bn_actor(N, 64, True, seed=6)
    norms = [a[0] for a in actor.actors] if per_agent else [actor[0]]
    f = dict(dtype=torch.float32, device=DEV)
    out = dict(obs=torch.empty((K, B, N, 6 * N), **f), reward=torch.empty((K, B, N), **f), indiv=torch.empty((K, B, N), **f),
               done=torch.zeros((K, B, N), dtype=torch.uint8, device=DEV), act=torch.empty((K, B, N, 2), **f))

    def run(tag):
        obs0 = _current_obs(env)
        obs, _, _, info = env.rollout_actor(K, actor, out=out)
        worst = bt.bn_fidelity(actor, _obs_before(obs0, obs, K), info["actions"])
        print("BNFIDELITY in-place per_agent=%d %s max err/bound = %.4f" % (per_agent, tag, worst))
        assert worst <= 1.0, "%s: max err / bound = %.3g" % (tag, worst)
        return info["actions"].clone()
    assert env.actor_path(actor) == "fused"
    first = run("first")
    bound = dict(env._roll_launchers)
    assert len(bound) == 1
    with torch.no_grad():
        for bn in norms:
            bn.running_mean.copy_(bn.running_mean + 0.3)
            bn.running_var.copy_(bn.running_var * 1.7 + 0.1)
    second = run("copy_")
    assert dict(env._roll_launchers) == bound, "the same buffers and tensors must reuse the bound launcher"
    assert not torch.equal(first, second)
    for i, bn in enumerate(norms):                                      # a trainer's state dict: other statistics, same tensors
        src = nn.BatchNorm1d(6 * N, eps=bn.eps, affine=bn.weight is not None)
        with torch.no_grad():
            src.running_mean.normal_(0.0, 0.4)
            src.running_var.uniform_(0.3, 2.0)
            if src.weight is not None:
                src.weight.uniform_(0.5, 1.5)
                src.bias.normal_(0.0, 0.3)
        ptr = bn.running_mean.data_ptr()
        bn.load_state_dict(src.state_dict())
        assert bn.running_mean.data_ptr() == ptr
    third = run("load_state_dict")
    assert dict(env._roll_launchers) == bound and not torch.equal(second, third)
    actor.train()
    assert env.actor_path(actor) == "host"
    actor.eval()
    assert env.actor_path(actor) == "fused"


@pytest.mark.parametrize("N,H,per_agent", [(9, 64, False), (27, 32, False), (16, 64, True)])
def test_host_paced_twin_at_step_0(N, H, per_agent):
    env = _env(N)
    actor = _pa_actor(N, H, seed=8) if per_agent else _bn_actor(N, H, True, seed=8)
    host = _Wrap(actor)
    assert env.actor_path(actor) == "fused" and env.actor_path(host) == "host"
    snap = env._snapshot()
    obs0 = _current_obs(env)
    fused = env.rollout_actor(K, actor)[3]["actions"].clone()
    env._restore(snap)
    paced = env.rollout_actor(K, host)[3]["actions"].clone()
    assert paced.shape == fused.shape == (K, B, N, 2)
    bound = _bound_at(actor, obs0, 2.0)
    diff = (paced[0].double() - fused[0].double()).abs()
    print("BNTWIN det N=%d H=%d per_agent=%d max diff/(2 bound) at step 0 = %.4f" % (N, H, per_agent, float((diff / bound).max())))
    assert bool((diff <= bound).all())
