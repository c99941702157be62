"""GPU tests of the recurrent actor rollout: `env.rollout_actor(K, actor, rnn_state=h)` with rMAPPO's policy (onpolicy's R_Actor:
the LayerNorm body - GRU - LayerNorm - Linear [- Tanh]), deterministic and as the mean of a GaussianActor, fused
(`fg_rollout_hd_actor_gru`, gru_actor_kernel / gru_sample_kernel) against an fp64 reference.

Fidelity bounds.  The reference is `copy.deepcopy(actor).double()`, its GRU step written out by hand, on the observation a step
acted on and on the fp32 state that went into it - both known exactly for a one-step launch, so fidelity is checked step by
step through K one-step launches that pass the state along (which the split test shows to be the K-step launch's bits).  The
body carries the LayerNorm actor's bound (test_gpu_actor_layernorm): an absolute error of about 1e-5 max(1, r1) max(1, r2) on
the GRU's input x, r1 / r2 the rows' fp64 rstd of the two hidden norms.  The GRU step maps an input error e to at most about
e |W_ih| row sums / 4 through the sigmoids and e |W_in| through the tanh - slopes at most 1 at these weights - and adds a few
ulp per gate; the state is bounded by 1, so it has no max(1, |h|) factor:
    |h32 - h64| <= 1e-5 * max(1, r1) * max(1, r2).
The norm after the GRU scales that by its row's rstd r3, and the head is a Linear as before:
    |a32 - a64| <= 1e-5 * max(1, |a64|) * max(1, r1) * max(1, r2) * max(1, r3).
1e-5 and the rstd factors are the LayerNorm test's; the state bound and r3 follow its error model.

The factor the step puts on e is in fact max(1, S_in, S_ir / 4, S_iz / 4), S the largest row sum of |W| of a gate's block of
weight_ih (tests/actor_fidelity.py, `gate_gain`): 4.9 to 6.8 at these weights, not 1.  The cases of this file keep the bound
above, without that gain - the measured figures sit far inside it; the cases with scaled GRU weights (test_gpu_actor_edges.py)
carry it.

Largest measured err / bound per case on MI355X (each test prints its figures, lines starting GRUFIDELITY / GRUTWIN, before it
asserts), action then state - 0.039 and 0.078 at most:
test_replay_determinism_split_fidelity (N, H, input norm, tanh): (3, 64, yes, yes) 0.017 0.041, (4, 64, no, yes) 0.008 0.024,
  (8, 64, yes, no) 0.019 0.039, (9, 64, no, no) 0.019 0.033, (16, 64, yes, yes) 0.018 0.046, (25, 64, no, yes) 0.015 0.039,
  (27, 64, yes, no) 0.024 0.078, (32, 64, no, no) 0.039 0.077, (9, 32, no, yes) 0.017 0.035, (27, 32, yes, no) 0.028 0.060
test_masking (either auto_reset): (9, 64) 0.010 0.025, (27, 32) 0.009 0.023
test_gaussian: (9, 64, yes, no) 0.016 0.032, (27, 64, no, yes) 0.025 0.054; host-paced twin over one step, diff / (2 bound):
  0.006 0.015 and 0.004 0.009
test_fresh_parameters_seen_by_bound_launcher: N = 9 0.018 0.043, N = 27 0.019 0.048
A figure above 1 is a finding to explain, not a bound to widen.

Host-paced twin.  The same modules with the base behind `Wrap` resolve to the host-paced loop.  Both paths evaluate the same
fp32 parameters on the same observation and state only at the first step of a launch, so the twin is compared over one step,
within twice the bounds (both sides carry them), and over all K steps where the actions are the noise itself (zeroed head):
there the two trajectories and log-probs are the same bits.
"""
import copy

import pytest
import torch

from formation_gym import GaussianActor, RecurrentActor, _native
from formation_gym.actor_rollout import FUSED_N
from tests.actor_fidelity import EDGE_EPS, TOL, rec_actor, rec_ref64 as _ref64, rec_step_errors as _step_errors
from tests.actor_testlib import (B, DEV, K, Wrap as _Wrap, clone as _clone, current_obs as _current_obs, env as _env,
                                 logp_formula as _logp_formula, noise_at as _noise_at, state as _state)

pytestmark = pytest.mark.gpu

# (N, H, input norm, tanh): every N at H = 64, alternating the input norm and the tanh, plus two shapes at H = 32
CASES = [(n, 64, i % 2 == 0, i % 4 < 2) for i, n in enumerate(FUSED_N)] + [(9, 32, False, True), (27, 32, True, False)]
nn = torch.nn


def _rec_actor(N, H, in_norm, tanh=False, seed=0, zero_head=False, eps=1e-5, wrap=False):
    """tests/actor_fidelity.py's `rec_actor` on DEV.  `wrap`: the base behind Wrap - the host-paced twin."""
    actor = rec_actor(N, H, in_norm, tanh, seed, zero_head, eps, device=DEV)
    return _twin(actor) if wrap else actor


def _twin(actor):
    """The same modules, the base behind a module the path rule does not recognise: runs host-paced."""
    return RecurrentActor(_Wrap(actor.base), actor.rnn, actor.norm, actor.head)


def _random_state(N, H, seed=11):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((B, N, H), generator=g) * 2 - 1).to(DEV)


def _one_steps(env, actor, h, steps, ref=None, eps_scale=None):
    """`steps` one-step launches passing the state `h` along (in place): stacked (actions, obs, rewards, done[, log_prob]) and
    the worst (action, state) err / bound against `ref` (None: not checked).  `eps_scale`: exp(log_std) of a Gaussian actor,
    whose mean is actions - eps_scale * fg_actor_noise."""
    acts, obss, rews, dones, logps = [], [], [], [], []
    worst = [0.0, 0.0]
    for _ in range(steps):
        obs0, h_in = _current_obs(env), h.clone()
        eps = _noise_at(env, 0) if eps_scale is not None else None
        obs, rew, done, info = env.rollout_actor(1, actor, rnn_state=h)
        assert info["rnn_state"] is h
        acts.append(info["actions"][0].clone()); obss.append(obs[0].clone()); rews.append(rew[0].clone())
        dones.append(done[0].clone())
        if "log_prob" in info:
            logps.append(info["log_prob"][0].clone())
        if ref is not None:
            mean = acts[-1] if eps is None else acts[-1].double() - eps_scale.double() * eps.double()
            a_err, h_err = _step_errors(ref, obs0, h_in, mean, h, dones[-1])
            worst = [max(worst[0], a_err), max(worst[1], h_err)]
    out = [torch.stack(t) for t in (acts, obss, rews, dones)]
    return out + ([torch.stack(logps)] if logps else []), worst


@pytest.mark.parametrize("N,H,in_norm,tanh", CASES)
def test_replay_determinism_split_fidelity(N, H, in_norm, tanh):
    env = _env(N)
    actor = _rec_actor(N, H, in_norm, tanh)
    assert env.actor_path(actor) == "fused"
    h0 = _random_state(N, H)
    snap = env._snapshot()
    h = h0.clone()
    obs, rew, done, info = _clone(env.rollout_actor(K, actor, rnn_state=h))
    state = _state(env)
    assert bool(done.any()), "no episode boundary inside the launch: nothing was masked"
    assert "log_prob" not in info and torch.equal(info["rnn_state"], h) and not torch.equal(h, h0)
    # replay through the open-loop rollout: the same bits
    env._restore(snap)
    r_obs, r_rew, r_done, r_info = env.rollout(info["actions"].clone())
    assert torch.equal(obs, r_obs) and torch.equal(rew, r_rew) and torch.equal(done, r_done)
    assert torch.equal(info["individual_reward"], r_info["individual_reward"])
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)
    # a second launch from the same snapshot and state: the same bits
    env._restore(snap)
    h2 = h0.clone()
    obs2, rew2, _, info2 = env.rollout_actor(K, actor, rnn_state=h2)
    assert torch.equal(info["actions"], info2["actions"]) and torch.equal(obs, obs2) and torch.equal(rew, rew2)
    assert torch.equal(h, h2)
    # K one-step launches that pass the state along: the same bits, and each step the fp64 actor on what it acted on
    env._restore(snap)
    h3 = h0.clone()
    (acts, obss, rews, dones), worst = _one_steps(env, actor, h3, K, copy.deepcopy(actor).double())
    assert torch.equal(acts, info["actions"]) and torch.equal(obss, obs) and torch.equal(rews, rew) and torch.equal(dones, done)
    assert torch.equal(h3, h)
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)
    # one 10 + 14 split
    env._restore(snap)
    h4 = h0.clone()
    first = _clone(env.rollout_actor(10, actor, rnn_state=h4))
    second = _clone(env.rollout_actor(14, actor, rnn_state=h4))
    assert torch.equal(torch.cat((first[3]["actions"], second[3]["actions"])), info["actions"])
    assert torch.equal(torch.cat((first[0], second[0])), obs) and torch.equal(torch.cat((first[1], second[1])), rew)
    assert torch.equal(h4, h)
    print("GRUFIDELITY det N=%d H=%d in_norm=%d tanh=%d max err/bound action = %.4f state = %.4f"
          % (N, H, in_norm, tanh, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, "max err / bound: action %.3g, state %.3g" % tuple(worst)


@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("N,H,in_norm", [(9, 64, True), (27, 32, False)])
def test_masking(N, H, in_norm, auto_reset):
    env = _env(N)
    env.auto_reset = auto_reset
    wl = int(env.world.world_length)
    env.world.step_count[::3] = wl - 1                          # this step ends a third of the episodes
    actor = _rec_actor(N, H, in_norm, tanh=True)
    assert env.actor_path(actor) == "fused"
    h = _random_state(N, H)
    (acts, obss, rews, dones), worst = _one_steps(env, actor, h, 1, copy.deepcopy(actor).double())
    done = dones[0]
    assert bool(done[::3].all()) and bool((~done).any()) and bool((done == done[:, :1]).all())
    assert not bool(h[::3].any()), "the state of the envs whose episode ended is not exactly zero"
    assert bool((h[~done] != 0).any(-1).all()), "a row that lives on was zeroed"
    print("GRUFIDELITY mask N=%d H=%d auto_reset=%d max err/bound action = %.4f state = %.4f"
          % (N, H, auto_reset, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, "max err / bound: action %.3g, state %.3g" % tuple(worst)


@pytest.mark.parametrize("N", [3, 27])
def test_tail_workgroup(N):
    """B = 5: fewer envs than one workgroup holds (64 at N = 3, 8 at N = 27).  The first five envs of the B = 133 batch built on
    the same seeds start from the same state and draw from the same streams: the same bits."""
    H, few = 64, 5
    actor = GaussianActor(_rec_actor(N, H, True, tanh=False), nn.Parameter(torch.tensor([-0.7, -0.2], device=DEV)))
    full, small = _env(N), _env(N, num_envs=few)
    assert small.actor_path(actor) == "fused"
    fw, fs, sw, ss = full.world, full.scenario, small.world, small.scenario
    for dst, src in ((sw.pos_x, fw.pos_x), (sw.pos_y, fw.pos_y), (sw.vel_x, fw.vel_x), (sw.vel_y, fw.vel_y),
                     (sw.step_count, fw.step_count), (ss.ideal_shape, fs.ideal_shape), (ss.ideal_vel, fs.ideal_vel)):
        dst.copy_(src[:few])                                     # the same initial state, whatever the reset drew
    h_full = _random_state(N, H)
    h_small = h_full[:few].clone()
    _, _, done, want = _clone(full.rollout_actor(K, actor, rnn_state=h_full))
    _, _, _, got = _clone(small.rollout_actor(K, actor, rnn_state=h_small))
    assert bool(done[:, :few].any())
    assert torch.equal(got["actions"], want["actions"][:, :few]) and torch.equal(got["log_prob"], want["log_prob"][:, :few])
    assert torch.equal(h_small, h_full[:few])


@pytest.mark.parametrize("N,H,in_norm,tanh", [(9, 64, True, False), (27, 64, False, True)])
def test_gaussian(N, H, in_norm, tanh):
    env = _env(N)
    log_std = nn.Parameter(torch.tensor([-0.5, 0.3], device=DEV))
    actor = GaussianActor(_rec_actor(N, H, in_norm, tanh), log_std)
    host = GaussianActor(_twin(actor.mean), log_std)
    assert env.actor_path(actor) == "fused" and env.actor_path(host) == "host"
    h0 = _random_state(N, H)
    snap = env._snapshot()
    eps = torch.stack([_noise_at(env, k) for k in range(K)])
    h = h0.clone()
    obs, rew, done, info = _clone(env.rollout_actor(K, actor, rnn_state=h))
    assert bool(done.any()) and info["log_prob"].shape == (K, B, N)
    # the draws are fg_actor_noise at each step's offset: the formula on them
    assert torch.allclose(info["log_prob"], _logp_formula(eps, log_std.detach()), rtol=1e-6, atol=0)
    # step by step: the same bits, and actions - exp(log_std) eps is the fp64 mean on what the step acted on
    env._restore(snap)
    h1 = h0.clone()
    (acts, obss, rews, dones, logps), worst = _one_steps(env, actor, h1, K, copy.deepcopy(actor.mean).double(),
                                                         torch.exp(log_std.detach()))
    assert torch.equal(acts, info["actions"]) and torch.equal(obss, obs) and torch.equal(logps, info["log_prob"])
    assert torch.equal(h1, h)
    print("GRUFIDELITY gauss N=%d H=%d in_norm=%d tanh=%d max err/bound action = %.4f state = %.4f"
          % (N, H, in_norm, tanh, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, "max err / bound: action %.3g, state %.3g" % tuple(worst)
    # the host-paced twin over one step from the same observation and state: twice the bounds
    env._restore(snap)
    obs0 = _current_obs(env)
    hf = h0.clone()
    _, _, d_f, i_f = _clone(env.rollout_actor(1, actor, rnn_state=hf))
    env._restore(snap)
    hh = h0.clone()
    res_h = env.rollout_actor(1, host, rnn_state=hh)
    assert res_h[3]["rnn_state"] is hh                            # before _clone, which copies info's tensors
    _, _, d_h, i_h = _clone(res_h)
    assert torch.equal(d_f, d_h)
    with torch.no_grad():
        a64, _, r1, r2, r3 = _ref64(copy.deepcopy(actor.mean).double(), obs0.double(), h0.double())
    base = 2 * TOL * torch.clamp(r1, min=1.0) * torch.clamp(r2, min=1.0)
    a_diff = (i_h["actions"][0].double() - i_f["actions"][0].double()).abs() / (base * torch.clamp(a64.abs(), min=1.0)
                                                                                 * torch.clamp(r3, min=1.0))
    h_diff = (hh.double() - hf.double()).abs() / base
    print("GRUTWIN N=%d H=%d one step, max diff/(2 bound) action = %.4f state = %.4f" % (N, H, float(a_diff.max()),
                                                                                      float(h_diff.max())))
    assert float(a_diff.max()) <= 1.0 and float(h_diff.max()) <= 1.0
    assert torch.equal(i_h["log_prob"], i_f["log_prob"])
    assert torch.equal(hh == 0, hf == 0)


@pytest.mark.parametrize("N,in_norm", [(9, True), (27, False)])
def test_gaussian_exact_noise_over_two_launches(N, in_norm):
    """A zeroed head: the actions are the noise itself, so the host-paced twin walks the same trajectory bit for bit."""
    H = 64
    env = _env(N)
    log_std = nn.Parameter(torch.zeros(2, device=DEV))
    actor = GaussianActor(_rec_actor(N, H, in_norm, zero_head=True), log_std)
    host = GaussianActor(_twin(actor.mean), log_std)
    assert env.actor_path(actor) == "fused" and env.actor_path(host) == "host"
    hf, hh = _random_state(N, H), _random_state(N, H)
    seen = []
    for launch in range(2):
        want = torch.stack([_noise_at(env, k) for k in range(K)])
        snap = env._snapshot()
        obs, rew, done, info = _clone(env.rollout_actor(K, actor, rnn_state=hf))
        state = _state(env)
        assert launch == 1 or bool(done.any())
        assert torch.equal(info["actions"], want), "launch %d: the actions are not fg_actor_noise at each step's offset" % launch
        assert torch.allclose(info["log_prob"], _logp_formula(want, torch.zeros(2, device=DEV)), rtol=1e-6, atol=0)
        seen.append(info["actions"])
        env._restore(snap)
        h_obs, h_rew, h_done, h_info = env.rollout_actor(K, host, rnn_state=hh)
        assert torch.equal(h_info["actions"], info["actions"]) and torch.equal(h_info["log_prob"], info["log_prob"])
        assert torch.equal(h_obs, obs) and torch.equal(h_rew, rew) and torch.equal(h_done, done)
        for a, b in zip(state, _state(env)):
            assert torch.equal(a, b)
        assert torch.equal(hh == 0, hf == 0)                     # the same rows masked by the last step
    assert not bool((seen[0] == seen[1]).all(-1).any()), "the second launch repeats draws of the first"


@pytest.mark.parametrize("N,in_norm", [(9, True), (27, False)])
def test_fresh_parameters_seen_by_bound_launcher(N, in_norm):
    H = 64
    env = _env(N)
    actor = _rec_actor(N, H, in_norm, tanh=True)
    f = dict(dtype=torch.float32, device=DEV)
    out = dict(obs=torch.empty((1, B, N, 6 * N), **f), reward=torch.empty((1, B, N), **f), indiv=torch.empty((1, B, N), **f),
               done=torch.zeros((1, B, N), dtype=torch.uint8, device=DEV), act=torch.empty((1, B, N, 2), **f))
    h0 = _random_state(N, H)
    h = h0.clone()
    snap = env._snapshot()
    obs0 = _current_obs(env)
    first = env.rollout_actor(1, actor, out=out, rnn_state=h)[3]["actions"].clone()
    bound = dict(env._roll_launchers)
    assert len(bound) == 1
    before = [p.detach().clone() for p in actor.parameters()]
    opt = torch.optim.SGD(actor.parameters(), lr=0.05)           # every parameter: body, GRU, norm and head
    a, hn = actor(torch.randn(7, 6 * N, device=DEV), torch.rand(7, H, device=DEV) * 2 - 1)
    (a.square().sum() + hn.square().sum()).backward()
    opt.step()
    for p in actor.rnn.parameters():
        assert p.grad is not None and bool(p.grad.abs().sum() > 0)
    assert all(not torch.equal(x, y) for x, y in zip(before, actor.parameters()))
    env._restore(snap)
    h.copy_(h0)
    _, _, done, info = env.rollout_actor(1, actor, out=out, rnn_state=h)
    assert dict(env._roll_launchers) == bound, "the same buffers, parameters and state must reuse the bound launcher"
    assert not torch.equal(first, info["actions"])
    worst = _step_errors(copy.deepcopy(actor).double(), obs0, h0, info["actions"][0], h, done[0])
    print("GRUFIDELITY fresh N=%d in_norm=%d max err/bound action = %.4f state = %.4f" % (N, in_norm, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, "max err / bound: action %.3g, state %.3g" % tuple(worst)


@pytest.mark.parametrize("N,H,in_norm,gaussian", [(9, 64, True, True), (25, 32, False, False)])
def test_c_abi_call_equals_rollout_actor(N, H, in_norm, gaussian):
    env = _env(N)
    mean = _rec_actor(N, H, in_norm, tanh=True, eps=EDGE_EPS)            # one eps per norm: the fields cannot be permuted
    log_std = nn.Parameter(torch.tensor([0.2, -0.4], device=DEV))
    actor = GaussianActor(mean, log_std) if gaussian else mean
    assert env.actor_path(actor) == "fused"
    h0 = _random_state(N, H)
    snap = env._snapshot()
    h = h0.clone()
    obs, rew, done, info = _clone(env.rollout_actor(K, actor, rnn_state=h))
    state = _state(env)
    env._restore(snap)
    f = dict(dtype=torch.float32, device=DEV)
    o = dict(obs=torch.empty((K, B, N, 6 * N), **f), reward=torch.empty((K, B, N), **f), indiv=torch.empty((K, B, N), **f),
             done=torch.zeros((K, B, N), dtype=torch.uint8, device=DEV), act=torch.empty((K, B, N, 2), **f),
             logp=torch.empty((K, B, N), **f))
    lins = [m for m in mean.base if isinstance(m, nn.Linear)] + [mean.head[0]]
    lns = [m for m in mean.base if isinstance(m, nn.LayerNorm)]
    fa = _native.FgActor(H, 1, *[t.data_ptr() for l in lins for t in (l.weight, l.bias)])
    hid = lns[-2:]
    fn = _native.FgActorNorm(lns[0].weight.data_ptr() if in_norm else None, lns[0].bias.data_ptr() if in_norm else None,
                             hid[0].weight.data_ptr(), hid[0].bias.data_ptr(), hid[1].weight.data_ptr(), hid[1].bias.data_ptr(),
                             lns[0].eps, hid[0].eps, hid[1].eps, 1 if in_norm else 0)
    g = mean.rnn
    fgru = _native.FgActorGru(g.weight_ih.data_ptr(), g.weight_hh.data_ptr(), g.bias_ih.data_ptr(), g.bias_hh.data_ptr(),
                              mean.norm.weight.data_ptr(), mean.norm.bias.data_ptr(), mean.norm.eps)
    hc = h0.clone()
    w, sc = env.world, env.scenario
    p = sc.params(w, True, env._launch_rng_offset(), o["obs"])
    rc = _native.load().fg_rollout_hd_actor_gru(
        p, fa, fn, fgru, log_std.data_ptr() if gaussian else None, B, N, K, w.pos_x.data_ptr(), w.pos_y.data_ptr(),
        w.vel_x.data_ptr(), w.vel_y.data_ptr(), o["act"].data_ptr(), sc.ideal_shape.data_ptr(), sc.ideal_vel.data_ptr(),
        w.step_count.data_ptr(), o["obs"].data_ptr(), o["reward"].data_ptr(), o["indiv"].data_ptr(), o["done"].data_ptr(),
        o["logp"].data_ptr() if gaussian else None, hc.data_ptr(), 1, _native.current_stream(DEV))
    _native.check(rc)
    torch.cuda.synchronize()
    assert torch.equal(o["act"], info["actions"]) and torch.equal(o["obs"], obs)
    assert torch.equal(o["indiv"], info["individual_reward"]) and torch.equal(o["done"].view(torch.bool), done)
    assert torch.equal((o["reward"] if env.shared_reward else o["indiv"]).unsqueeze(-1), rew)
    if gaussian:
        assert torch.equal(o["logp"], info["log_prob"])
    assert torch.equal(hc, h)
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)


def test_state_argument():
    N, H = 9, 64
    env = _env(N)
    actor = _rec_actor(N, H, True)
    snap = env._snapshot()
    # None: a fresh zero state per call, handed back
    _, _, _, info = _clone(env.rollout_actor(K, actor))
    from_none = info["rnn_state"]
    assert from_none.shape == (B, N, H) and from_none.dtype == torch.float32 and bool(from_none.any())
    env._restore(snap)
    h = torch.zeros((B, N, H), device=DEV)
    ptr = h.data_ptr()
    _, _, _, info2 = env.rollout_actor(K, actor, rnn_state=h)
    assert info2["rnn_state"] is h and h.data_ptr() == ptr                        # updated in place
    assert torch.equal(h, from_none) and torch.equal(info2["actions"], info["actions"])
    # the host-paced loop handles the state the same way
    env._restore(snap)
    hh = torch.zeros((B, N, H), device=DEV)
    twin = _twin(actor)
    assert env.actor_path(twin) == "host"
    _, _, _, info3 = env.rollout_actor(2, twin, rnn_state=hh)
    assert info3["rnn_state"] is hh and bool(hh.any())
    # a state the launch cannot take, and a state without a recurrent actor
    plain = nn.Sequential(*actor.base, nn.Linear(H, 2).to(DEV))
    assert env.actor_path(plain) == "fused"
    with pytest.raises(ValueError):
        env.rollout_actor(K, plain, rnn_state=h)
    with pytest.raises(ValueError):
        env.rollout_actor(K, GaussianActor(plain, nn.Parameter(torch.zeros(2, device=DEV))), rnn_state=h)
    for bad in (h[:, :, :32], h.double(), h[:-1].clone(), h.cpu()):
        with pytest.raises(ValueError):
            env.rollout_actor(K, actor, rnn_state=bad)
