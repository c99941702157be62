"""GPU tests of `env.rollout_actor`: the closed loop of a learned MLP actor inside the rollout kernel (`fg_rollout_hd_actor`)
and its host-paced twin.

Actor fidelity bound.  Each layer of the fused actor is a k-ordered fp32 fma chain (v_mfma_f32_16x16x4_f32 for layers 1 and
2, v_fma_f32 for layer 3): its error against fp64 is about 1e-7 * sum_k |w_k x_k| per output (one rounding per product,
cdna_hip_programming 'FP32-input MFMA'), and ReLU does not amplify it.  With PyTorch's default initialisation scaled by
ACT_SCALE the sums |w x| stay below ~20 for every layer at these inputs (observations are O(1)), so an output carries at most
a few 1e-6 of absolute error, and tanh (slope <= 1) does not enlarge it: 1e-5 abs for tanh outputs, 1e-5 max(1, |a|) without
tanh.  The physics is checked bit for bit: replaying the recorded actions through `env.rollout` must give the same state,
observations, rewards and done flags.
"""
import copy

import pytest
import torch

from formation_gym.actor_rollout import FUSED_N
from formation_gym.vec_env import FormationVecEnv
from tests.actor_testlib import (B, DEV, K, clone as _clone, current_obs as _current_obs, env as _env, hand_loop as _hand_loop,
                                 obs_before as _obs_before, scaled_mlp, state as _state)

pytestmark = pytest.mark.gpu

TOL = 1e-5
CASES = [(n, 64) for n in FUSED_N] + [(9, 32), (9, 128), (27, 32), (27, 128)]


def _actor(N, H, tanh=True, seed=0):
    return scaled_mlp(6 * N, H, tanh, seed)


def _check_fidelity(actor, obs_before, acts, tanh, steps=None):
    """acts [K,B,N,2] vs the actor in fp64 on obs_before[k] (the observation step k acted on)."""
    ref = copy.deepcopy(actor).double()
    for k in (range(len(acts)) if steps is None else steps):
        with torch.no_grad():
            want = ref(obs_before[k].double())
        got = acts[k].double()
        bound = TOL if tanh else TOL * torch.clamp(want.abs(), min=1.0)
        err = (got - want).abs()
        assert bool((err <= bound).all()), "step %d: max err %.3g" % (k, float(err.max()))


@pytest.mark.parametrize("N,H", CASES)
def test_replay_fidelity_determinism(N, H):
    env = _env(N)
    actor = _actor(N, H, tanh=(H != 128))       # H = 128 runs the five-module actor (no tanh)
    assert env.actor_path(actor) == "fused"
    snap = env._snapshot()
    obs0 = _current_obs(env)
    obs, rew, done, info = _clone(env.rollout_actor(K, actor))
    state = _state(env)
    assert bool(done.any()), "no episode boundary inside the launch"
    # 1. replay through the open-loop rollout: the same bits
    env._restore(snap)
    r_obs, r_rew, r_done, r_info = env.rollout(info["actions"].clone())
    assert torch.equal(obs, r_obs) and torch.equal(rew, r_rew) and torch.equal(done, r_done)
    assert torch.equal(info["individual_reward"], r_info["individual_reward"])
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)
    # 2. the actions are the actor on the observations the kernel wrote
    _check_fidelity(actor, _obs_before(obs0, obs, K), info["actions"], tanh=(H != 128))
    # 3. two launches from the same snapshot: the same bits
    env._restore(snap)
    obs2, _, _, info2 = env.rollout_actor(K, actor)
    assert torch.equal(info["actions"], info2["actions"]) and torch.equal(obs, obs2)


@pytest.mark.parametrize("N", [9, 27])
def test_fresh_weights_seen_by_bound_launcher(N):
    env = _env(N)
    actor = _actor(N, 64)
    f = dict(dtype=torch.float32, device=DEV)
    out = dict(obs=torch.empty((K, B, N, 6 * N), **f), reward=torch.empty((K, B, N), **f), indiv=torch.empty((K, B, N), **f),
               done=torch.zeros((K, B, N), dtype=torch.uint8, device=DEV), act=torch.empty((K, B, N, 2), **f))
    env.rollout_actor(K, actor, out=out)
    bound = dict(env._roll_launchers)
    opt = torch.optim.SGD(actor.parameters(), lr=0.05)
    actor(torch.randn(7, 6 * N, device=DEV)).square().sum().backward()
    opt.step()
    obs0 = _current_obs(env)
    obs, _, _, info = env.rollout_actor(K, actor, out=out)
    assert dict(env._roll_launchers) == bound, "the same buffers and parameters must reuse the bound launcher"
    _check_fidelity(actor, _obs_before(obs0, obs, K), info["actions"], tanh=True)


@pytest.mark.parametrize("N", [9, 27])
def test_layouts_and_options(N):
    env = _env(N)
    actor = _actor(N, 64)
    snap = env._snapshot()
    obs0 = _current_obs(env)
    ref = _clone(env.rollout_actor(20, actor, out=False))
    state = _state(env)
    # obs_every = 5: the same actions, every fifth observation, replayable
    env._restore(snap)
    obs5, rew5, done5, info5 = _clone(env.rollout_actor(20, actor, obs_every=5))
    assert torch.equal(info5["actions"], ref[3]["actions"]) and torch.equal(obs5, ref[0][4::5])
    assert torch.equal(rew5, ref[1]) and torch.equal(done5, ref[2])
    env._restore(snap)
    r_obs, r_rew, _, _ = env.rollout(info5["actions"].clone(), obs_every=5)
    assert torch.equal(r_obs, obs5) and torch.equal(r_rew, rew5)
    _check_fidelity(actor, _obs_before(obs0, ref[0], 20), info5["actions"], tanh=True)
    # a padded env pitch
    env._restore(snap)
    D = 6 * N
    pitch = N * D + 34
    f = dict(dtype=torch.float32, device=DEV)
    flat = torch.zeros((20 * B * pitch,), **f)
    out = dict(obs=flat.as_strided((20, B, N, D), (B * pitch, pitch, D, 1)), reward=torch.empty((20, B, N), **f),
               indiv=torch.empty((20, B, N), **f), done=torch.zeros((20, B, N), dtype=torch.uint8, device=DEV),
               act=torch.empty((20, B, N, 2), **f))
    obs_p, _, _, info_p = env.rollout_actor(20, actor, out=out)
    assert torch.equal(obs_p, ref[0]) and torch.equal(info_p["actions"], ref[3]["actions"])
    assert not bool(flat.view(20, B, pitch)[:, :, N * D:].any()), "the pad was written"
    # the vec-env wrapper runs the same launch
    env._restore(snap)
    venv = FormationVecEnv(env)
    v_obs, _, _, v_info = venv.rollout_actor(20, actor)
    assert torch.equal(v_obs, ref[0]) and torch.equal(v_info["actions"], ref[3]["actions"])
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)


def test_per_agent_props_run_host_paced():
    N = 9
    env = _env(N)
    env.world.agents[1].initial_mass = 2.0         # World.agent_props: a per-agent table the fused kernel does not read
    actor = _actor(N, 64)
    assert env.actor_path(actor) == "host"
    snap = env._snapshot()
    obs, rew, _, info = env.rollout_actor(6, actor)
    env._restore(snap)
    acts, h_obs, h_rew = _hand_loop(env, actor, 6)
    assert torch.equal(info["actions"], acts) and torch.equal(obs, h_obs) and torch.equal(rew, h_rew)


@pytest.mark.parametrize("N", [9, 27])
def test_unfusable_actor_runs_host_paced(N):
    env = _env(N)
    torch.manual_seed(1)
    actor = torch.nn.Sequential(torch.nn.Linear(6 * N, 64), torch.nn.GELU(), torch.nn.Linear(64, 2)).to(DEV)
    assert env.actor_path(actor) == "host"
    snap = env._snapshot()
    obs, rew, done, info = env.rollout_actor(8, actor)
    env._restore(snap)
    acts, h_obs, h_rew = _hand_loop(env, actor, 8)
    assert torch.equal(info["actions"], acts) and torch.equal(obs, h_obs) and torch.equal(rew, h_rew)
