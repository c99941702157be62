"""GPU tests of `env.rollout_actor` in the landmark scenarios (basic_formation_env, formation_hd_partial_env,
formation_hd_partial_range_env, formation_hd_obs_env): the learned actor inside the one-env-per-lane rollout kernel
(`fg_rollout_scenario_actor`: scn_lane_actor / scn_lane_actor_gauss) and its host-paced twin.

Physics: bit for bit - replaying the recorded actions through `env.rollout` from the same snapshot must give the same
observations, rewards, done flags and final state (the fused kernel's step is scn_lane_kernel's source text).

Actor fidelity bound: the one of tests/test_gpu_actor_rollout.py, whose derivation carries over because the layers are
evaluated in the same order (k-ascending fp32 fma chains on v_mfma_f32_16x16x4_f32 for layers 1 and 2, v_fma_f32 for layer 3)
on a narrower input: D <= 28 against 6N = 18 ... 192.  Checked on the CPU for D in {18, 22, 24, 26, 28}, H in {32, 64} and
inputs up to |3| with PyTorch's default initialisation scaled by ACT_SCALE: max sum |w x| per layer 11.8 (the derivation
allows 20), torch's own fp32 forward within 6e-7 of fp64.  So 1e-5 abs for tanh outputs, 1e-5 max(1, |a|) without tanh, on
every (step, env, agent).  The Gaussian variant is compared on a - exp(log_std) eps, eps replayed from `fg_actor_noise` at
each step's offset, and its log-prob with -(eps_0^2 + eps_1^2) / 2 - sum(log_std) - log(2 pi) at 1e-6.
"""
import copy
import math

import pytest
import torch

import formation_gym
from formation_gym import placement
from formation_gym.actor_rollout import GaussianActor
from formation_gym.core import Wall
from formation_gym.vec_env import FormationVecEnv
from tests.actor_testlib import (B, DEV, K, Wrap as _Wrap, clone as _clone, current_obs as _current_obs, env as _make_env,
                                 hand_loop as _hand_loop, noise_at as _noise_at, obs_before as _obs_before, scaled_mlp as _mlp)

pytestmark = pytest.mark.gpu

B_BIG = 300              # more than 256 envs: several workgroups, the last one ragged
TOL = 1e-5
# the seven shapes of the one-env-per-lane kernel: (scenario, agents)
SHAPES = [("basic_formation_env", 3), ("formation_hd_partial_env", 5), ("formation_hd_partial_env", 3),
          ("formation_hd_partial_range_env", 4), ("formation_hd_partial_range_env", 3),
          ("formation_hd_obs_env", 4), ("formation_hd_obs_env", 3)]
REFERENCE = SHAPES[:2] + [SHAPES[3], SHAPES[5]]


def _env(name, N, seed=3, num_envs=B):
    return _make_env(N, seed, num_envs, name)


def _actor(env, H, tanh=True, gauss=False, seed=0):
    mean = _mlp(env._out["obs"].shape[-1], H, tanh, seed)
    if not gauss:
        return mean
    return GaussianActor(mean, torch.nn.Parameter(torch.tensor([-0.5, 0.3], device=DEV)))


def _state(env):
    w = env.world
    return [t.clone() for t in (w.pos_x, w.pos_y, w.vel_x, w.vel_y, w.landmark_pos, w.obstacle_pos, w.obstacle_vel, w.step_count)]


def _check_fidelity(mean, obs_before, acts, tanh, steps=None, what=""):
    """acts [K,B,N,2] (the mean's part of the action) vs the actor in fp64 on obs_before[k] (the observation step k acted
    on); every (env, agent) of every step."""
    ref = copy.deepcopy(mean).double()
    worst = 0.0
    for k in (range(len(acts)) if steps is None else steps):
        with torch.no_grad():
            want = ref(obs_before[k].double())
        got = acts[k].double()
        bound = torch.full_like(want, TOL) if tanh else TOL * torch.clamp(want.abs(), min=1.0)
        err = (got - want).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all()), "%s step %d: max err %.3g" % (what, k, float(err.max()))
    print("%s fidelity: worst err / bound %.3f" % (what, worst))


def _replay_and_fidelity(env, actor, H, tanh, gauss, what):
    """Tests 6, 7 and the determinism half of 9 for one env and actor."""
    assert env.actor_path(actor) == "fused"
    snap = env._snapshot()
    obs0 = _current_obs(env)
    eps = [_noise_at(env, k) for k in range(K)] if gauss else None
    obs, rew, done, info = _clone(env.rollout_actor(K, actor))
    state = _state(env)
    N = env.num_agents
    assert tuple(info["actions"].shape) == (K, env.num_envs, N, 2) and tuple(obs.shape[:3]) == (K, env.num_envs, N)
    assert bool(done.any()) and not bool(done.all()), "no episode boundary inside the launch"
    assert bool(torch.isfinite(info["actions"]).all()) and bool(torch.isfinite(obs).all())
    # replay through the open-loop rollout: the same bits
    env._restore(snap)
    r_obs, r_rew, r_done, r_info = env.rollout(info["actions"].clone(), out=False)
    assert torch.equal(obs, r_obs), what
    assert torch.equal(rew, r_rew) and torch.equal(done, r_done)
    assert torch.equal(info["individual_reward"], r_info["individual_reward"])
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)
    # the actions are the actor on the observations the kernel composed
    before = _obs_before(obs0, obs, K)
    if gauss:
        ls = actor.log_std.detach()
        std = torch.exp(ls.double())
        mean_part = torch.stack([info["actions"][k].double() - std * eps[k].double() for k in range(K)])
        _check_fidelity(actor.mean, before, mean_part, tanh, what=what)
        for k in range(K):
            e = eps[k].double()
            want = -0.5 * (e[..., 0] ** 2 + e[..., 1] ** 2) - float(ls.double().sum()) - math.log(2.0 * math.pi)
            err = (info["log_prob"][k].double() - want).abs()
            assert float(err.max()) <= 1e-6 * max(1.0, float(want.abs().max())), "log_prob step %d: %.3g" % (k, float(err.max()))
    else:
        _check_fidelity(actor, before, info["actions"], tanh, what=what)
    # two launches from the same snapshot: the same bits
    env._restore(snap)
    obs2, rew2, _, info2 = env.rollout_actor(K, actor)
    assert torch.equal(info["actions"], info2["actions"]) and torch.equal(obs, obs2) and torch.equal(rew, rew2)
    if gauss:
        assert torch.equal(info["log_prob"], info2["log_prob"])


@pytest.mark.parametrize("gauss", [False, True])
@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("name,N", SHAPES)
def test_replay_fidelity_determinism(name, N, H, gauss):
    env = _env(name, N)
    tanh = H == 64                  # both output forms over the sweep
    actor = _actor(env, H, tanh=tanh, gauss=gauss)
    _replay_and_fidelity(env, actor, H, tanh, gauss, "%s N=%d H=%d gauss=%d" % (name, N, H, gauss))


@pytest.mark.parametrize("gauss", [False, True])
@pytest.mark.parametrize("name,N", REFERENCE)
def test_batch_above_256_envs(name, N, gauss):
    env = _env(name, N, num_envs=B_BIG)
    actor = _actor(env, 64, tanh=not gauss, gauss=gauss, seed=1)
    _replay_and_fidelity(env, actor, 64, not gauss, gauss, "%s N=%d B=%d gauss=%d" % (name, N, B_BIG, gauss))


@pytest.mark.parametrize("name,N", REFERENCE)
def test_host_and_fused_paths_match(name, N):
    env = _env(name, N)
    fused = _actor(env, 64, gauss=True)
    host = GaussianActor(_Wrap(fused.mean), fused.log_std)
    assert env.actor_path(fused) == "fused" and env.actor_path(host) == "host"
    snap = env._snapshot()
    _, _, _, f_info = _clone(env.rollout_actor(K, fused))
    env._restore(snap)
    _, _, _, h_info = _clone(env.rollout_actor(K, host))
    # step 0: both means within the fidelity bound of fp64, hence within twice the bound of each other; the same eps draws
    # at every step (log_prob is a function of eps alone)
    a0, b0 = f_info["actions"][0].double(), h_info["actions"][0].double()
    assert float((a0 - b0).abs().max()) <= 2 * TOL * max(1.0, float(b0.abs().max()))
    assert tuple(f_info["log_prob"].shape) == tuple(h_info["log_prob"].shape) == (K, B, N)
    assert torch.allclose(f_info["log_prob"], h_info["log_prob"], rtol=1e-6, atol=1e-6)
    # deterministic actors: step 0 within the bound
    env._restore(snap)
    d_f = env.rollout_actor(1, fused.mean, out=False)[3]["actions"].clone()
    env._restore(snap)
    d_h = env.rollout_actor(1, _Wrap(fused.mean))[3]["actions"]
    assert float((d_f - d_h).abs().max()) <= 2 * TOL


@pytest.mark.parametrize("name,N", [SHAPES[0], SHAPES[5]])
def test_weights_and_log_std_read_in_place(name, N):
    env = _env(name, N)
    actor = _actor(env, 64, gauss=True)
    D = env._out["obs"].shape[-1]
    f = dict(dtype=torch.float32, device=DEV)
    out = dict(obs=torch.empty((K, B, N, D), **f), reward=torch.empty((K, B, N), **f), indiv=torch.empty((K, B, N), **f),
               done=torch.zeros((K, B, N), dtype=torch.uint8, device=DEV), act=torch.empty((K, B, N, 2), **f),
               log_prob=torch.empty((K, B, N), **f))
    snap = env._snapshot()
    first = _clone(env.rollout_actor(K, actor, out=out))
    bound = dict(env._roll_launchers)
    assert len(bound) == 1
    with torch.no_grad():                              # an optimizer-style update in place, and a new log_std
        for i, p in enumerate(actor.mean.parameters()):
            p.add_(0.01 * (i + 1) * torch.ones_like(p))
        actor.log_std.copy_(torch.tensor([0.1, -0.2], device=DEV))
    env._restore(snap)
    obs0 = _current_obs(env)
    eps = [_noise_at(env, k) for k in range(K)]
    obs, _, _, info = env.rollout_actor(K, actor, out=out)
    assert dict(env._roll_launchers) == bound, "the same buffers and parameters must reuse the bound launcher"
    assert not torch.equal(first[3]["actions"], info["actions"])
    std = torch.exp(actor.log_std.detach().double())
    mean_part = torch.stack([info["actions"][k].double() - std * eps[k].double() for k in range(K)])
    _check_fidelity(actor.mean, _obs_before(obs0, obs, K), mean_part, True, what="updated weights")
    want = -0.5 * (eps[0].double() ** 2).sum(-1) - (0.1 - 0.2) - math.log(2.0 * math.pi)
    assert float((info["log_prob"][0].double() - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("name,N", [SHAPES[0], SHAPES[1], SHAPES[5]])
def test_layouts(name, N):
    env = _env(name, N)
    actor = _actor(env, 64)
    snap = env._snapshot()
    obs0 = _current_obs(env)
    ref = _clone(env.rollout_actor(K, actor, out=False))
    state = _state(env)
    # obs_every = 3: the same actions, every third observation, replayable
    env._restore(snap)
    obs3, rew3, done3, info3 = _clone(env.rollout_actor(K, actor, obs_every=3))
    assert tuple(obs3.shape[:1]) == (K // 3,)
    assert torch.equal(info3["actions"], ref[3]["actions"]) and torch.equal(obs3, ref[0][2::3])
    assert torch.equal(rew3, ref[1]) and torch.equal(done3, ref[2])
    env._restore(snap)
    r_obs, r_rew, _, _ = env.rollout(info3["actions"].clone(), obs_every=3, out=False)
    assert torch.equal(r_obs, obs3) and torch.equal(r_rew, rew3)
    _check_fidelity(actor, _obs_before(obs0, ref[0], K), info3["actions"], True, what="obs_every=3")
    # caller-supplied buffers
    env._restore(snap)
    D = env._out["obs"].shape[-1]
    f = dict(dtype=torch.float32, device=DEV)
    out = dict(obs=torch.empty((K, B, N, D), **f), reward=torch.empty((K, B, N), **f), indiv=torch.empty((K, B, N), **f),
               done=torch.zeros((K, B, N), dtype=torch.uint8, device=DEV), act=torch.empty((K, B, N, 2), **f))
    obs_c, rew_c, _, info_c = env.rollout_actor(K, actor, out=out)
    assert obs_c.data_ptr() == out["obs"].data_ptr() and info_c["actions"].data_ptr() == out["act"].data_ptr()
    assert torch.equal(obs_c, ref[0]) and torch.equal(info_c["actions"], ref[3]["actions"]) and torch.equal(rew_c, ref[1])
    # the landmark scenarios write contiguous observation buffers only
    env._restore(snap)
    pitch = N * D + 34
    flat = torch.zeros((K * B * pitch,), **f)
    with pytest.raises(ValueError):
        env.rollout_actor(K, actor, out=dict(out, obs=flat.as_strided((K, B, N, D), (B * pitch, pitch, D, 1))))
    # out=None without placement means fresh tensors
    env._restore(snap)
    env.default_placed = False
    a = env.rollout_actor(K, actor)
    assert torch.equal(a[0], ref[0]) and torch.equal(a[3]["actions"], ref[3]["actions"])
    env._restore(snap)
    b = env.rollout_actor(K, actor)
    assert a[0].data_ptr() != b[0].data_ptr()
    env.default_placed = True
    # the vec-env wrapper runs the same launch
    env._restore(snap)
    venv = FormationVecEnv(env)
    v_obs, v_rew, _, v_info = venv.rollout_actor(K, actor)
    assert torch.equal(v_obs, ref[0]) and torch.equal(v_info["actions"], ref[3]["actions"]) and torch.equal(v_rew, ref[1])
    for x, y in zip(state, _state(env)):
        assert torch.equal(x, y)


def test_placed_buffers_at_the_benchmark_shape():
    Bn, Kn = 65536, 20
    env = formation_gym.make_env("basic_formation_env", False, 3, num_envs=Bn, device=DEV)
    env.seed(5)
    env.reset()
    env.auto_reset = True
    D = env._out["obs"].shape[-1]
    assert Kn * Bn * 3 * D * 4 >= placement.MIN_PROBE_BYTES
    actor = _actor(env, 64)
    assert env.actor_path(actor) == "fused" and env.default_placed
    snap = env._snapshot()
    ref = _clone(env.rollout_actor(Kn, actor, out=False))
    env._restore(snap)
    obs, rew, done, info = env.rollout_actor(Kn, actor)       # probes, restores the env, then runs the measured call
    rep = env.placement
    assert rep is not None and rep.get("tried", 0) >= 1
    # probed, unless the report says that no second candidate could be made (free memory): {"tried": 1, "probed": False}
    assert rep.get("probed") or rep.get("tried") == 1, rep
    assert rep["buffer_MB"] >= placement.MIN_PROBE_BYTES / 1e6
    assert torch.equal(obs, ref[0]) and torch.equal(rew, ref[1]) and torch.equal(done, ref[2])
    assert torch.equal(info["actions"], ref[3]["actions"])
    ptr = obs.data_ptr()
    obs2, _, _, info2 = env.rollout_actor(Kn, actor)
    assert obs2.data_ptr() == ptr and info2["actions"].data_ptr() == info["actions"].data_ptr()


@pytest.mark.parametrize("case", ["basic4", "h128", "walls"])
def test_fallbacks_run_host_paced(case):
    N = 4 if case == "basic4" else 3
    env = _env("basic_formation_env", N)
    if case == "walls":
        env.world.walls = [Wall("V", -0.8, (-1.0, 1.0), 0.1), Wall("H", 0.7, (-0.5, 0.5), 0.2)]
    actor = _actor(env, 128 if case == "h128" else 64)
    assert env.actor_path(actor) == "host"
    D = env._out["obs"].shape[-1]
    snap = env._snapshot()
    obs, rew, done, info = env.rollout_actor(6, actor)
    assert tuple(obs.shape) == (6, B, N, D) and tuple(rew.shape) == (6, B, N, 1) and tuple(done.shape) == (6, B, N)
    assert tuple(info["actions"].shape) == (6, B, N, 2) and tuple(info["individual_reward"].shape) == (6, B, N)
    env._restore(snap)
    acts, h_obs, h_rew = _hand_loop(env, actor, 6)
    assert torch.equal(info["actions"], acts) and torch.equal(obs, h_obs) and torch.equal(rew, h_rew)
