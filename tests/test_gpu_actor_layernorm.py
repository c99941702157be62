"""GPU tests of the LayerNorm actor rollout: `env.rollout_actor(K, actor)` with the MAPPO trainers' actor (onpolicy's
MLPBase: [LayerNorm -] Linear - ReLU - LayerNorm - Linear - ReLU - LayerNorm - Linear [- Tanh]), deterministic and as the mean
of a GaussianActor, fused (`fg_rollout_hd_actor_norm`, ln_actor_kernel / ln_sample_kernel) against an fp64 reference.

Actor fidelity bound.  The reference is `copy.deepcopy(actor).double()` on the observation each step acted on.  Each Linear
carries the project's actor bound (test_gpu_actor_rollout: about 1e-7 * sum |w x| per output, below 1e-5 max(1, |a|) at these
weights).  A hidden LayerNorm maps an absolute error e of its input row to about e * rstd * |gamma| (the mean and the variance
move by O(e) too, which the same factor covers) and adds a few ulp of its own output; the input norm sees exact inputs and
only adds rounding.  With r1, r2 the rows' rstd of the two hidden norms in the fp64 evaluation, every action must meet
    |a32 - a64| <= 1e-5 * max(1, |a64|) * max(1, r1) * max(1, r2).
Largest measured err / bound per case on MI355X (each test prints its figure before it asserts) - 0.11 at most, i.e. about
1e-6 max(1, |a|) r1 r2:
test_replay_determinism_fidelity (N, H, input norm, tanh): (3, 64, yes, yes) 0.026, (4, 64, no, yes) 0.023, (8, 64, yes, no) 0.047,
  (9, 64, no, no) 0.055, (16, 64, yes, yes) 0.052, (25, 64, no, yes) 0.055, (27, 64, yes, no) 0.058, (32, 64, no, no) 0.072,
  (9, 32, no, yes) 0.024, (27, 32, yes, no) 0.093
test_gaussian_mean_fidelity_replay_and_host_twin, actions - exp(log_std) eps: (9, 64, yes, no) 0.047, (27, 64, no, yes) 0.054,
  (4, 32, yes, no) 0.032, (32, 64, yes, no) 0.063; host-paced twin at step 0, diff / (2 bound): 0.018, 0.011, 0.012, 0.028
test_fresh_parameters_seen_by_bound_launcher: N = 9 0.054, N = 27 0.110
test_dead_rows_return_beta (no rstd factor in the bound): (9, 64, yes) 0.009, (27, 32, no) 0.004, (16, 64, yes) 0.016

Host-paced twin.  Both paths evaluate the same fp32 modules on the same observation only at the first step of a launch: from
step 1 on each path acts on the observation its own (slightly different) action produced, which the error model of one actor
evaluation does not cover.  The twin is therefore compared at step 0, within twice the bound (both sides carry it), and over
all K steps where the actions are the noise itself (zeroed mean): there the two trajectories are the same bits.
"""
import copy

import pytest
import torch

from formation_gym import GaussianActor, _native
from formation_gym.actor_rollout import FUSED_N
from tests.actor_fidelity import EDGE_EPS, TOL, ln_actor, ln_fidelity as _fidelity, ln_ref64 as _ref64
from tests.actor_testlib import (B, DEV, K, Wrap as _Wrap, clone as _clone, current_obs as _current_obs, env as _env,
                                 logp_formula as _logp_formula, noise_at as _noise_at, obs_before as _obs_before, state as _state)

pytestmark = pytest.mark.gpu

# (N, H, input norm, tanh): every N at H = 64, alternating with and without the input norm, plus two shapes at H = 32
CASES = [(n, 64, i % 2 == 0, i % 4 < 2) for i, n in enumerate(FUSED_N)] + [(9, 32, False, True), (27, 32, True, False)]
nn = torch.nn


def _ln_actor(*args, **kwargs):
    """tests/actor_fidelity.py's `ln_actor` on DEV."""
    return ln_actor(*args, device=DEV, **kwargs)


@pytest.mark.parametrize("N,H,in_norm,tanh", CASES)
def test_replay_determinism_fidelity(N, H, in_norm, tanh):
    env = _env(N)
    actor = _ln_actor(N, H, in_norm, tanh)
    # 1. the new form runs fused
    assert env.actor_path(actor) == "fused"
    snap = env._snapshot()
    obs0 = _current_obs(env)
    obs, rew, done, info = _clone(env.rollout_actor(K, actor))
    state = _state(env)
    assert bool(done.any()), "no episode boundary inside the launch"
    assert "log_prob" not in info
    # 2. replay through the open-loop rollout: the same bits
    env._restore(snap)
    r_obs, r_rew, r_done, r_info = env.rollout(info["actions"].clone())
    assert torch.equal(obs, r_obs) and torch.equal(rew, r_rew) and torch.equal(done, r_done)
    assert torch.equal(info["individual_reward"], r_info["individual_reward"])
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)
    # 3. two launches from the same snapshot: the same bits
    env._restore(snap)
    obs2, rew2, _, info2 = env.rollout_actor(K, actor)
    assert torch.equal(info["actions"], info2["actions"]) and torch.equal(obs, obs2) and torch.equal(rew, rew2)
    # 4. the actions are the fp64 actor on the observations the kernel wrote
    worst = _fidelity(actor, _obs_before(obs0, obs, K), info["actions"])
    print("LNFIDELITY det N=%d H=%d in_norm=%d tanh=%d max err/bound = %.4f" % (N, H, in_norm, tanh, worst))
    assert worst <= 1.0, "max err / bound = %.3g" % worst


@pytest.mark.parametrize("N,H,in_norm", [(9, 64, True), (27, 32, False), (16, 64, True)])
def test_dead_rows_return_beta(N, H, in_norm):
    """b1 = -100: every first-layer ReLU output is zero, so the first hidden norm sees rows of zeros - variance 0, centred
    values exactly 0, rstd = 1 / sqrt(eps) - and must return beta exactly.  No rstd factor in the bound."""
    env = _env(N)
    actor = _ln_actor(N, H, in_norm)
    lin1 = [m for m in actor if isinstance(m, nn.Linear)][0]
    with torch.no_grad():
        lin1.bias.fill_(-100.0)
    assert env.actor_path(actor) == "fused"
    obs0 = _current_obs(env)
    obs, _, _, info = _clone(env.rollout_actor(K, actor))
    before = _obs_before(obs0, obs, K)
    ref = copy.deepcopy(actor).double()
    with torch.no_grad():
        for k in range(K):
            assert not bool(_ref64(ref, before[k].double())[3].any()), "the premise: every first-layer output is dead"
    assert bool(torch.isfinite(info["actions"]).all())
    worst = _fidelity(actor, before, info["actions"], rstd_factor=False)
    print("LNFIDELITY dead N=%d H=%d in_norm=%d max err/bound = %.4f" % (N, H, in_norm, worst))
    assert worst <= 1.0, "max err / bound (no rstd factor) = %.3g" % worst
    # beta exactly: with dead rows the actor is a constant, the same bits for every row and step
    flat = info["actions"].reshape(-1, 2)
    assert bool((flat == flat[0]).all())


@pytest.mark.parametrize("N,in_norm", [(9, True), (27, False)])
def test_gaussian_exact_noise_over_two_launches(N, in_norm):
    env = _env(N)
    actor = GaussianActor(_ln_actor(N, 64, in_norm, zero_head=True), nn.Parameter(torch.zeros(2, device=DEV)))
    host = GaussianActor(_Wrap(actor.mean), actor.log_std)
    assert env.actor_path(actor) == "fused" and env.actor_path(host) == "host"
    seen = []
    for launch in range(2):
        want = torch.stack([_noise_at(env, k) for k in range(K)])
        snap = env._snapshot()
        obs, rew, done, info = _clone(env.rollout_actor(K, actor))
        state = _state(env)
        assert launch == 1 or bool(done.any()), "no episode boundary inside the launch"
        acts, logp = info["actions"], info["log_prob"]
        assert acts.shape == (K, B, N, 2) and logp.shape == (K, B, N)
        assert torch.equal(acts, want), "launch %d: the actions are not fg_actor_noise at each step's offset" % launch
        assert torch.allclose(logp, _logp_formula(acts, torch.zeros(2, device=DEV)), rtol=1e-6, atol=0)
        seen.append(acts)
        # the host-paced twin from the same state: the same draws, the same trajectory, the same log_prob bits
        env._restore(snap)
        h_obs, h_rew, h_done, h_info = env.rollout_actor(K, host)
        assert torch.equal(h_info["actions"], acts)
        assert torch.equal(h_obs, obs) and torch.equal(h_rew, rew) and torch.equal(h_done, done)
        n_diff = int((h_info["log_prob"] != logp).sum())
        print("LNLOGP N=%d launch %d: host / fused log_prob differ in %d of %d" % (N, launch, n_diff, logp.numel()))
        assert torch.equal(h_info["log_prob"], logp)
        for a, b in zip(state, _state(env)):
            assert torch.equal(a, b)
    assert not bool((seen[0] == seen[1]).all(-1).any()), "the second launch repeats draws of the first"


@pytest.mark.parametrize("N,H,in_norm,tanh", [(9, 64, True, False), (27, 64, False, True), (4, 32, True, False),
                                             (32, 64, True, False)])
def test_gaussian_mean_fidelity_replay_and_host_twin(N, H, in_norm, tanh):
    env = _env(N)
    log_std = nn.Parameter(torch.tensor([-0.5, 0.3], device=DEV))
    actor = GaussianActor(_ln_actor(N, H, in_norm, tanh), log_std)
    host = GaussianActor(_Wrap(actor.mean), log_std)
    assert env.actor_path(actor) == "fused" and env.actor_path(host) == "host"
    snap = env._snapshot()
    obs0 = _current_obs(env)
    eps = torch.stack([_noise_at(env, k) for k in range(K)])
    obs, rew, done, info = _clone(env.rollout_actor(K, actor))
    state = _state(env)
    assert bool(done.any())
    # the recorded actions replay to the same bits
    env._restore(snap)
    r_obs, r_rew, r_done, _ = env.rollout(info["actions"].clone())
    assert torch.equal(obs, r_obs) and torch.equal(rew, r_rew) and torch.equal(done, r_done)
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)
    # determinism
    env._restore(snap)
    _, _, _, info2 = _clone(env.rollout_actor(K, actor))
    assert torch.equal(info["actions"], info2["actions"]) and torch.equal(info["log_prob"], info2["log_prob"])
    # the same eps draws and log-probs as the plain Gaussian actor's: the formula on fg_actor_noise
    assert torch.allclose(info["log_prob"], _logp_formula(eps, log_std.detach()), rtol=1e-6, atol=0)
    # actions - exp(log_std) eps is the mean: bound 4
    mean32 = info["actions"].double() - torch.exp(log_std.detach().double()) * eps.double()
    worst = _fidelity(actor.mean, _obs_before(obs0, obs, K), mean32)
    print("LNFIDELITY gauss N=%d H=%d in_norm=%d tanh=%d max err/bound = %.4f" % (N, H, in_norm, tanh, worst))
    assert worst <= 1.0, "max err / bound = %.3g" % worst
    # the host-paced twin draws the same eps; at step 0 both act on the same observation: twice bound 4 (module docstring)
    env._restore(snap)
    _, _, _, h_info = env.rollout_actor(K, host)
    ref = copy.deepcopy(actor.mean).double()
    with torch.no_grad():
        want, r1, r2, _ = _ref64(ref, obs0.double())
    bound = 2 * TOL * torch.clamp(want.abs(), min=1.0) * torch.clamp(r1, min=1.0) * torch.clamp(r2, min=1.0)
    diff = (h_info["actions"][0].double() - info["actions"][0].double()).abs()
    print("LNTWIN N=%d H=%d max diff/bound at step 0 = %.4f" % (N, H, float((diff / bound).max())))
    assert bool((diff <= bound).all())
    assert torch.allclose(h_info["log_prob"][0], info["log_prob"][0], rtol=1e-6, atol=0)


@pytest.mark.parametrize("N,in_norm", [(9, True), (27, False)])
def test_fresh_parameters_seen_by_bound_launcher(N, in_norm):
    env = _env(N)
    actor = _ln_actor(N, 64, in_norm, tanh=True)
    f = dict(dtype=torch.float32, device=DEV)
    out = dict(obs=torch.empty((K, B, N, 6 * N), **f), reward=torch.empty((K, B, N), **f), indiv=torch.empty((K, B, N), **f),
               done=torch.zeros((K, B, N), dtype=torch.uint8, device=DEV), act=torch.empty((K, B, N, 2), **f))
    first = env.rollout_actor(K, actor, out=out)[3]["actions"].clone()
    bound = dict(env._roll_launchers)
    assert len(bound) == 1
    before = [p.detach().clone() for p in actor.parameters()]
    opt = torch.optim.SGD(actor.parameters(), lr=0.05)           # the weights and the norms' gamma / beta
    actor(torch.randn(7, 6 * N, device=DEV)).square().sum().backward()
    opt.step()
    norms = [m for m in actor if isinstance(m, nn.LayerNorm)]
    for m in norms:
        assert m.weight.grad is not None and bool(m.weight.grad.abs().sum() > 0) and bool(m.bias.grad.abs().sum() > 0)
    assert all(not torch.equal(a, b) for a, b in zip(before, actor.parameters()))
    obs0 = _current_obs(env)
    obs, _, _, info = env.rollout_actor(K, actor, out=out)
    assert dict(env._roll_launchers) == bound, "the same buffers and parameters must reuse the bound launcher"
    worst = _fidelity(actor, _obs_before(obs0, obs, K), info["actions"])
    print("LNFIDELITY fresh N=%d in_norm=%d max err/bound = %.4f" % (N, in_norm, worst))
    assert worst <= 1.0, "max err / bound = %.3g" % worst
    assert not torch.equal(first, info["actions"])


@pytest.mark.parametrize("N,H,in_norm,gaussian", [(9, 64, True, True), (25, 32, False, False)])
def test_c_abi_call_equals_rollout_actor(N, H, in_norm, gaussian):
    env = _env(N)
    mean = _ln_actor(N, H, in_norm, tanh=True, eps=EDGE_EPS)             # one eps per norm: the fields cannot be permuted
    log_std = nn.Parameter(torch.tensor([0.2, -0.4], device=DEV))
    actor = GaussianActor(mean, log_std) if gaussian else mean
    assert env.actor_path(actor) == "fused"
    snap = env._snapshot()
    obs, rew, done, info = _clone(env.rollout_actor(K, actor))
    state = _state(env)
    env._restore(snap)
    f = dict(dtype=torch.float32, device=DEV)
    o = dict(obs=torch.empty((K, B, N, 6 * N), **f), reward=torch.empty((K, B, N), **f), indiv=torch.empty((K, B, N), **f),
             done=torch.zeros((K, B, N), dtype=torch.uint8, device=DEV), act=torch.empty((K, B, N, 2), **f),
             logp=torch.empty((K, B, N), **f))
    lins = [m for m in mean if isinstance(m, nn.Linear)]
    lns = [m for m in mean if isinstance(m, nn.LayerNorm)]
    fa = _native.FgActor(H, 1, *[t.data_ptr() for l in lins for t in (l.weight, l.bias)])
    hid = lns[-2:]
    fn = _native.FgActorNorm(lns[0].weight.data_ptr() if in_norm else None, lns[0].bias.data_ptr() if in_norm else None,
                             hid[0].weight.data_ptr(), hid[0].bias.data_ptr(), hid[1].weight.data_ptr(), hid[1].bias.data_ptr(),
                             lns[0].eps, hid[0].eps, hid[1].eps, 1 if in_norm else 0)
    w, sc = env.world, env.scenario
    p = sc.params(w, True, env._launch_rng_offset(), o["obs"])
    rc = _native.load().fg_rollout_hd_actor_norm(
        p, fa, fn, log_std.data_ptr() if gaussian else None, B, N, K, w.pos_x.data_ptr(), w.pos_y.data_ptr(),
        w.vel_x.data_ptr(), w.vel_y.data_ptr(), o["act"].data_ptr(), sc.ideal_shape.data_ptr(), sc.ideal_vel.data_ptr(),
        w.step_count.data_ptr(), o["obs"].data_ptr(), o["reward"].data_ptr(), o["indiv"].data_ptr(), o["done"].data_ptr(),
        o["logp"].data_ptr() if gaussian else None, 1, _native.current_stream(DEV))
    _native.check(rc)
    torch.cuda.synchronize()
    assert torch.equal(o["act"], info["actions"]) and torch.equal(o["obs"], obs)
    assert torch.equal(o["indiv"], info["individual_reward"]) and torch.equal(o["done"].view(torch.bool), done)
    assert torch.equal((o["reward"] if env.shared_reward else o["indiv"]).unsqueeze(-1), rew)
    if gaussian:
        assert torch.equal(o["logp"], info["log_prob"])
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)
