"""GPU tests of the edges of the LayerNorm and recurrent actor rollouts that tests/test_gpu_actor_layernorm.py and
tests/test_gpu_actor_recurrent.py cannot see: one eps per norm (the kernels read four fields - nw.eps0 / eps1 / eps2, gw.eps3 -
that the same value in all of them cannot tell apart), norms without gamma or beta and Linears without bias (the NULL -> 1 / 0
branches of the preloads), saturated and overflowing GRU gates with state entries that are exactly 0 or +-1, an nn.GRU member,
`obs_every` > 1 and dead rows in the recurrent actor.  The builders, references, bounds, the gate gain and the mutants are
tests/actor_fidelity.py's (its docstring derives them); tests/test_actor_fidelity_cpu.py shows on the CPU that these parameter
sets leave a right actor a factor of ten and put every mutant ten bounds away.

Every fidelity case runs one-step launches that pass the state along, so that each step is compared with the fp64 reference
on the observation and the fp32 state it acted on; 8 steps, the episode boundary of `actor_testlib.env` being at step 7.  The
rows of `edge_state` that are exactly 0, +1 or -1 go into the kernel once, at the first of the eight steps: from the second
step on the state is the kernel's own output (exact zeros return only in the rows a step masked).  Each prints its largest
err / bound (a line starting EDGEFIDELITY) before it asserts err / bound <= 1.

Largest measured err / bound on MI355X (action, state for the recurrent actor):
test_recurrent_distinct_eps: (9, 64) 0.012 0.028, (27, 32) 0.012 0.020, Gaussian (3, 32) 0.016 0.027; the weakest mutant on the
  env's own observations is 325 bounds away (unbiased_variance; the weakest eps swap 844)
test_layernorm_distinct_eps: (9, 64) 0.039, (32, 64) 0.051; weakest mutant 239 (unbiased_variance)
test_recurrent_absent_norm_parameters: no_affine (9, 64) 0.011 0.027, (27, 32) 0.030 0.040; mixed 0.011 0.029, 0.024 0.044
test_layernorm_absent_parameters: (9, 64) no_affine 0.024, mixed 0.029, mixed_no_linear_bias 0.030; Gaussian (27, 32) 0.060,
  0.069, 0.047
test_recurrent_saturated_gates (gain 19.6 to 28.2): (9, 64) 0.0012 0.0061, (9, 32) 0.0011 0.0065, (32, 64) 0.0016 0.0084,
  (32, 32) 0.0033 0.0137
test_recurrent_overflowing_gates (gain 183 and 134, 3700 and 7484 r / z pre-activations beyond 90 over the 8 steps): (9, 64)
  0.0031 0.0140, (32, 32) 0.0036 0.0355
test_recurrent_dead_rows: (9, 64) 0.0001 0.0001, without the rstd factors 0.0098 0.0098; (27, 32) 0.0001 0.0001 and 0.0063 0.0067
"""
import copy

import pytest
import torch

from formation_gym import GaussianActor
from tests.actor_fidelity import (EDGE_SETS, NORM_BIAS_ARG, TOL, edge_state, gate_gain, ln_actor, ln_fidelity,
                                  mutant_name, mutant_ratios, rec_actor, rec_ref64, rec_step_errors)
from tests.actor_testlib import (B, DEV, K, clone as _clone, current_obs as _current_obs, env as _env, noise_at as _noise_at,
                                 state as _state)

pytestmark = pytest.mark.gpu

nn = torch.nn
STEPS = 8


def _state_for(N, H):
    return edge_state((B, N, H)).to(DEV)


def _need_norm_bias(name):
    if "mixed" in name and not NORM_BIAS_ARG:
        pytest.skip("this torch's LayerNorm has no `bias` argument: a norm with gamma and without beta cannot be built")


def _rec_steps(env, actor, h, steps, gain=False):
    """`steps` one-step launches of the (Gaussian or deterministic) recurrent `actor` passing the state `h` along in place: the
    worst (action, state) err / bound against the fp64 mean on what each step acted on, whether a step ended an episode, and the
    (observation, state) pairs the steps acted on."""
    gaussian = isinstance(actor, GaussianActor)
    mean_mod = actor.mean if gaussian else actor
    ref = copy.deepcopy(mean_mod).double()
    scale = torch.exp(actor.log_std.detach().double()) if gaussian else None
    worst, any_done, seen = [0.0, 0.0], False, []
    for _ in range(steps):
        obs0, h_in = _current_obs(env), h.clone()
        eps = _noise_at(env, 0) if gaussian else None
        _, _, done, info = env.rollout_actor(1, actor, rnn_state=h)
        assert info["rnn_state"] is h
        act = info["actions"][0]
        mean = act.double() - scale * eps.double() if gaussian else act
        a_err, h_err = rec_step_errors(ref, obs0, h_in, mean, h, done[0], gain=gain)
        worst = [max(worst[0], a_err), max(worst[1], h_err)]
        any_done = any_done or bool(done.any())
        seen.append((obs0, h_in))
    assert any_done, "no episode boundary inside the steps: nothing was masked"
    return worst, seen


def _ln_steps(env, actor, steps):
    """`steps` one-step launches of the (Gaussian or deterministic) LayerNorm `actor`: the worst err / bound of the mean, and
    the observations the steps acted on."""
    gaussian = isinstance(actor, GaussianActor)
    scale = torch.exp(actor.log_std.detach().double()) if gaussian else None
    before, means = [], []
    for _ in range(steps):
        before.append(_current_obs(env))
        eps = _noise_at(env, 0) if gaussian else None
        act = env.rollout_actor(1, actor)[3]["actions"][0]
        means.append(act.double() - scale * eps.double() if gaussian else act.clone())
    return ln_fidelity(actor.mean if gaussian else actor, before, means), before


def _assert_mutants_visible(tag, actor, seen):
    """Each reference mutant, on the inputs the launches acted on (first and last step), is at least 10 bounds from the true
    reference there too.  The reference alone: no kernel output enters."""
    for obs0, h_in in (seen[0], seen[-1]):
        ratios = mutant_ratios(actor, obs0, h_in)
        weakest = min(ratios, key=ratios.get)
        print("EDGEMUTANT %s weakest on the env's observations: %s %.1f" % (tag, mutant_name(weakest), ratios[weakest]))
        assert ratios[weakest] >= 10.0, "the env's observations cannot see %s" % mutant_name(weakest)


# ---- distinct eps ----
@pytest.mark.parametrize("N,H,in_norm,gaussian", [(9, 64, True, False), (27, 32, False, False), (3, 32, True, True)])
def test_recurrent_distinct_eps(N, H, in_norm, gaussian):
    env = _env(N)
    mean = rec_actor(N, H, in_norm, tanh=not gaussian, device=DEV, **EDGE_SETS["eps"])
    actor = GaussianActor(mean, nn.Parameter(torch.tensor([-0.5, 0.3], device=DEV))) if gaussian else mean
    assert env.actor_path(actor) == "fused"
    worst, seen = _rec_steps(env, actor, _state_for(N, H), STEPS)
    print("EDGEFIDELITY rec eps N=%d H=%d in_norm=%d gaussian=%d max err/bound action = %.4f state = %.4f"
          % (N, H, in_norm, gaussian, worst[0], worst[1]))
    _assert_mutants_visible("rec N=%d H=%d" % (N, H), mean, seen)
    assert worst[0] <= 1.0 and worst[1] <= 1.0, "max err / bound: action %.3g, state %.3g" % tuple(worst)


@pytest.mark.parametrize("N,H,in_norm", [(9, 64, True), (32, 64, True)])
def test_layernorm_distinct_eps(N, H, in_norm):
    env = _env(N)
    actor = ln_actor(N, H, in_norm, tanh=True, device=DEV, **EDGE_SETS["eps"])
    assert env.actor_path(actor) == "fused"
    worst, before = _ln_steps(env, actor, STEPS)
    print("EDGEFIDELITY ln eps N=%d H=%d in_norm=%d max err/bound = %.4f" % (N, H, in_norm, worst))
    _assert_mutants_visible("ln N=%d H=%d" % (N, H), actor, [(before[0], None), (before[-1], None)])
    assert worst <= 1.0, "max err / bound = %.3g" % worst


# ---- absent parameters ----
@pytest.mark.parametrize("name", ["no_affine", "mixed"])
@pytest.mark.parametrize("N,H,in_norm", [(9, 64, True), (27, 32, True)])
def test_recurrent_absent_norm_parameters(N, H, in_norm, name):
    _need_norm_bias(name)
    env = _env(N)
    actor = rec_actor(N, H, in_norm, tanh=True, device=DEV, **EDGE_SETS[name])
    fused = env._resolve_actor(actor)
    assert env.actor_path(actor) == "fused" and fused is not None
    absent = [t is None for n in tuple(fused.norms) + (fused.gru.norm,) for t in n[:2]]
    assert absent == ([True] * 8 if name == "no_affine" else [True, True, False, True, True, True, False, False])
    worst, _ = _rec_steps(env, actor, _state_for(N, H), STEPS)
    print("EDGEFIDELITY rec %s N=%d H=%d max err/bound action = %.4f state = %.4f" % (name, N, H, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, "max err / bound: action %.3g, state %.3g" % tuple(worst)


@pytest.mark.parametrize("name", ["no_affine", "mixed", "mixed_no_linear_bias"])
@pytest.mark.parametrize("N,H,in_norm,gaussian", [(9, 64, True, False), (27, 32, True, True)])
def test_layernorm_absent_parameters(N, H, in_norm, gaussian, name):
    _need_norm_bias(name)
    env = _env(N)
    mean = ln_actor(N, H, in_norm, tanh=not gaussian, device=DEV, **EDGE_SETS[name])
    actor = GaussianActor(mean, nn.Parameter(torch.tensor([0.2, -0.4], device=DEV))) if gaussian else mean
    fused = env._resolve_actor(actor)
    assert env.actor_path(actor) == "fused" and fused is not None
    absent = [t is None for n in fused.norms for t in n[:2]]
    assert absent == ([True] * 6 if name == "no_affine" else [True, True, False, True, True, True])
    assert [t is None for t in fused.members[0][1::2]] == [name == "mixed_no_linear_bias"] * 3
    worst, _ = _ln_steps(env, actor, STEPS)
    print("EDGEFIDELITY ln %s N=%d H=%d gaussian=%d max err/bound = %.4f" % (name, N, H, gaussian, worst))
    assert worst <= 1.0, "max err / bound = %.3g" % worst


# ---- saturated gates ----
@pytest.mark.parametrize("N,H,in_norm", [(9, 64, True), (9, 32, False), (32, 64, False), (32, 32, True)])
def test_recurrent_saturated_gates(N, H, in_norm):
    """GRU weights times 6 (a third of the r / z pre-activations beyond 4, the largest near 20), states with rows of exact 0,
    +1 and -1: the bounds with the gate gain."""
    env = _env(N)
    actor = rec_actor(N, H, in_norm, tanh=True, device=DEV, **EDGE_SETS["saturated"])
    assert env.actor_path(actor) == "fused"
    worst, _ = _rec_steps(env, actor, _state_for(N, H), STEPS, gain=True)
    print("EDGEFIDELITY rec saturated N=%d H=%d gain=%.2f max err/bound action = %.4f state = %.4f"
          % (N, H, gate_gain(copy.deepcopy(actor).double()), worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, "max err / bound: action %.3g, state %.3g" % tuple(worst)


@pytest.mark.parametrize("N,H,in_norm", [(9, 64, True), (32, 32, False)])
def test_recurrent_overflowing_gates(N, H, in_norm):
    """GRU weights times 40: pre-activations beyond +-90, where expf(-x) of the sigmoid is inf on one side and 0 on the other.
    Everything stays finite, the state stays in [-1, 1], the masked rows are exactly zero, and the bounds with the gate gain
    hold."""
    env = _env(N)
    actor = rec_actor(N, H, in_norm, tanh=False, device=DEV, **EDGE_SETS["overflow"])
    assert env.actor_path(actor) == "fused"
    h = _state_for(N, H)
    ref = copy.deepcopy(actor).double()
    worst, beyond = [0.0, 0.0], 0
    for _ in range(STEPS):
        obs0, h_in = _current_obs(env), h.clone()
        _, _, done, info = env.rollout_actor(1, actor, rnn_state=h)
        act, done = info["actions"][0], done[0]
        assert bool(torch.isfinite(act).all()) and bool(torch.isfinite(h).all())
        assert float(h.abs().max()) <= 1.0
        assert not bool(h[done].any()), "a finished episode's state is not exactly zero"
        a_err, h_err = rec_step_errors(ref, obs0, h_in, act, h, done, gain=True)
        worst = [max(worst[0], a_err), max(worst[1], h_err)]
        with torch.no_grad():                                       # the premise, from the reference alone
            x = ref.base(obs0.double())
            w_ih, w_hh, b_ih, b_hh = ref.gru_parameters()
            pre = (x @ w_ih.T + b_ih + h_in.double() @ w_hh.T + b_hh)[..., :2 * H]
            beyond += int((pre.abs() > 90).sum())
    assert beyond > 0, "the premise: some r / z pre-activations beyond 90"
    print("EDGEFIDELITY rec overflow N=%d H=%d gain=%.2f (%d pre-activations beyond 90) max err/bound action = %.4f state = %.4f"
          % (N, H, gate_gain(ref), beyond, worst[0], worst[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, "max err / bound: action %.3g, state %.3g" % tuple(worst)


# ---- an nn.GRU member ----
@pytest.mark.parametrize("N,H,in_norm", [(9, 64, True), (27, 32, False)])
def test_gru_member_gives_the_grucell_bits(N, H, in_norm):
    env = _env(N)
    cell = rec_actor(N, H, in_norm, tanh=True, device=DEV, **EDGE_SETS["eps"])
    gru = rec_actor(N, H, in_norm, tanh=True, gru=True, device=DEV, **EDGE_SETS["eps"])
    assert isinstance(gru.rnn, nn.GRU) and isinstance(cell.rnn, nn.GRUCell)
    assert env.actor_path(cell) == "fused" and env.actor_path(gru) == "fused"
    h0 = _state_for(N, H)
    snap = env._snapshot()
    h_c = h0.clone()
    obs, rew, done, info = _clone(env.rollout_actor(K, cell, rnn_state=h_c))
    state = _state(env)
    assert bool(done.any())
    env._restore(snap)
    h_g = h0.clone()
    obs_g, rew_g, done_g, info_g = env.rollout_actor(K, gru, rnn_state=h_g)
    assert torch.equal(info_g["actions"], info["actions"]) and torch.equal(obs_g, obs) and torch.equal(rew_g, rew)
    assert torch.equal(done_g, done) and torch.equal(h_g, h_c) and not torch.equal(h_g, h0)
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)


# ---- obs_every ----
@pytest.mark.parametrize("kind,N,H,in_norm", [("rec", 9, 64, True), ("ln", 27, 32, False)])
def test_obs_every(kind, N, H, in_norm):
    """K = 20, obs_every = 5: the actions, log-probs and final state of obs_every = 1 from the same snapshot, every fifth
    observation, and the open-loop replay `rollout(actions, obs_every=5)` gives the same again."""
    KK, every = 20, 5
    env = _env(N)
    build = rec_actor if kind == "rec" else ln_actor
    actor = GaussianActor(build(N, H, in_norm, device=DEV, **EDGE_SETS["eps"]), nn.Parameter(torch.tensor([-0.5, 0.3], device=DEV)))
    assert env.actor_path(actor) == "fused"
    h0 = _state_for(N, H) if kind == "rec" else None
    state_kw = lambda h: {} if h is None else {"rnn_state": h}
    snap = env._snapshot()
    h1 = None if h0 is None else h0.clone()
    obs, rew, done, info = _clone(env.rollout_actor(KK, actor, **state_kw(h1)))
    state = _state(env)
    assert bool(done.any()) and obs.shape[0] == KK
    env._restore(snap)
    h5 = None if h0 is None else h0.clone()
    obs5, rew5, done5, info5 = _clone(env.rollout_actor(KK, actor, obs_every=every, **state_kw(h5)))
    assert obs5.shape == (KK // every,) + tuple(obs.shape[1:])
    assert torch.equal(obs5, obs[every - 1::every])
    assert torch.equal(info5["actions"], info["actions"]) and torch.equal(info5["log_prob"], info["log_prob"])
    assert torch.equal(rew5, rew) and torch.equal(done5, done)
    assert torch.equal(info5["individual_reward"], info["individual_reward"])
    if h0 is not None:
        assert torch.equal(h5, h1) and not torch.equal(h5, h0)
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)
    env._restore(snap)
    r_obs, r_rew, r_done, _ = env.rollout(info5["actions"].clone(), obs_every=every)
    assert torch.equal(r_obs, obs5) and torch.equal(r_rew, rew5) and torch.equal(r_done, done5)
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)


# ---- dead rows ----
@pytest.mark.parametrize("N,H,in_norm", [(9, 64, True), (27, 32, False)])
def test_recurrent_dead_rows(N, H, in_norm):
    """b1 = b2 = -100: every ReLU output is zero, so both hidden norms see rows of zeros - variance 0, centred values exactly
    0, rstd = 1 / sqrt(eps) - and the GRU's input x is beta2 exactly, for every row.  With eps = 1e-2 in both hidden norms
    (r1 = r2 = 10) the usual bound is 1e-3, which is loose here: x carries no error at all, so the step is also held to the
    bound without the rstd factors, as test_gpu_actor_layernorm.py's dead rows are."""
    env = _env(N)
    actor = rec_actor(N, H, in_norm, tanh=True, eps=(1e-3, 1e-2, 1e-2, 1e-1), device=DEV)
    lins = [m for m in actor.base if isinstance(m, nn.Linear)]
    with torch.no_grad():
        for lin in lins:
            lin.bias.fill_(-100.0)
    assert env.actor_path(actor) == "fused"
    ref = copy.deepcopy(actor).double()
    beta2 = [m for m in ref.base if isinstance(m, nn.LayerNorm)][-1].bias
    g = torch.Generator().manual_seed(4)
    h = (torch.rand((1, 1, H), generator=g) * 2 - 1).expand(B, N, H).contiguous().to(DEV)      # one state for every row
    worst, tight = [0.0, 0.0], [0.0, 0.0]
    for step in range(STEPS):
        obs0, h_in = _current_obs(env), h.clone()
        with torch.no_grad():
            x64 = ref.base(obs0.double())
            a64, h64, r1, r2, r3 = rec_ref64(ref, obs0.double(), h_in.double())
        assert bool((x64 == beta2).all()), "the premise: x is beta2 exactly"
        assert float((r2 - 10.0).abs().max()) <= 1e-12 and float((r1 - 10.0).abs().max()) <= 1e-12
        _, _, done, info = env.rollout_actor(1, actor, rnn_state=h)
        act, done = info["actions"][0], done[0]
        a_err, h_err = rec_step_errors(ref, obs0, h_in, act, h, done)
        worst = [max(worst[0], a_err), max(worst[1], h_err)]
        live = ~done
        bound_a = TOL * a64.abs().clamp(min=1.0) * r3.clamp(min=1.0)
        tight = [max(tight[0], float(((act.double() - a64).abs() / bound_a).max())),
                 max(tight[1], float((((h.double() - h64).abs() / TOL)[live]).max()))]
        if step == 0:                                   # the same x and the same state in every row: the same bits out
            flat_a, flat_h = act.reshape(-1, 2), h[live]
            assert bool((flat_a == flat_a[0]).all()) and bool((flat_h == flat_h[0]).all())
    print("EDGEFIDELITY rec dead N=%d H=%d max err/bound action = %.4f state = %.4f; without the rstd factors %.4f, %.4f"
          % (N, H, worst[0], worst[1], tight[0], tight[1]))
    assert worst[0] <= 1.0 and worst[1] <= 1.0, "max err / bound: action %.3g, state %.3g" % tuple(worst)
    assert tight[0] <= 1.0 and tight[1] <= 1.0, "max err / bound without rstd factors: action %.3g, state %.3g" % tuple(tight)
