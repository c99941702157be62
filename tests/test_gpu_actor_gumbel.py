"""GPU tests of the Gumbel member of the fused actor rollouts - MADDPG's discrete actions:
`env.rollout_actor(K, GumbelSoftmaxActor)` in the action modes FG_ACT_ONEHOT5 and FG_ACT_INDEX (`fg_rollout_hd_actor_gumbel`,
`fg_rollout_hd_actor_gumbel_per_agent`: gumbel_actor_kernel, pa_gumbel_actor_kernel, bn_gumbel_actor_kernel,
pa_bn_gumbel_actor_kernel), its host-paced twin and the helpers `fg_actor_gumbel` / `fg_actor_gumbel_pick`, against the fp64
reference of tests/actor_gumbel_testlib.py (semantics, bounds and mutants: that module's docstring;
tests/test_actor_gumbel_cpu.py shows that these inputs tell the mutants apart and that the reference alone keeps the exempt share
under the cap).

Inputs: env_index_base = 3, a 64-bit seed, a launch base offset of 2^32 - 2 (steps 1 and 2 of a K = 3 launch carry into the high
word), world_length = 2 with auto_reset (an episode ends inside the launch), and the shapes of `gt.CASES` - 3 x 70 (a second
workgroup with 6 live envs), 4 x 70 (group lanes exactly full), 9 x 20 (a half-empty last pass), 27 x 11 (half-full agent-major
tiles), 32 x 9 (the last slot of the per-agent table); H = 64 for the four forms everywhere, H = 32 at 9 x 20 and 27 x 11, H = 128
once each for the forms without a BatchNorm; both modes at 9 x 20, one elsewhere.

Bounds (derived: the testlib's docstring).  Every draw lies within gamma_j = 2^-21 (1 + max(1, |g_j|)) of the fp64 reference; an
index is compared outside the band eta = 2 beta + 2 max_j gamma_j + 2^-17 (exploring) or 2 beta (not exploring), which may hold
at most 1 % of a case's rows; the decoded action equals the decode of the index the launch itself returned on every row.
Run with `pytest -m gpu`; `-s` prints each case's measured figures (the largest |g32 - g64| / gamma, the exempt shares).
"""
import numpy as np
import pytest
import torch

import formation_gym
from formation_gym import GumbelSoftmaxActor, _native
from tests import actor_gumbel_testlib as gt
from tests.actor_testlib import DEV, Wrap as _Wrap, clone as _clone, current_obs as _current_obs, obs_before as _obs_before, \
    state as _state

pytestmark = pytest.mark.gpu

K = gt.K


def _env(N, B, mode, base=gt.BASE):
    sc = formation_gym.load_scenario("formation_hd_env")
    world = sc.make_world(N, num_envs=B, device=DEV)
    env = formation_gym.MultiAgentEnv(world, sc.reset_world, sc.reward, sc.observation, discrete_action=(mode == gt.ONEHOT5))
    env.discrete_action_input = mode == gt.INDEX
    env.seed(3)
    env.reset()
    env.auto_reset = True
    env.world.world_length = 2
    env.scenario._seed = gt.SEED                 # what `seed()` stores, without the host streams a 64-bit seed cannot key
    env.scenario.env_base = base
    env._rng_offset = gt.OFFSET - 1              # the next launch draws at OFFSET
    assert env._launch_rng_offset() == gt.OFFSET and env._action_mode() == mode
    return env


def _np(t):
    return t.detach().cpu().numpy()


def _rollout(env, actor, steps=K, **kw):
    return _clone(env.rollout_actor(steps, actor, out=False, **kw))


_REF = {}


def _draws(B, N):
    """The reference's g [K, B, N, 5] of the tests' launch: computed once per shape, never modified."""
    if (B, N) not in _REF:
        g = gt.launch_gumbels(gt.SEED, gt.BASE, B, N, gt.OFFSET, K)
        g.setflags(write=False)
        _REF[(B, N)] = g
    return _REF[(B, N)]


def _reference(actor, form, obs0, obs, B, N):
    """(logits [K, B, N, 5], beta [K, B, N]) of the fp64 actor on the observation each step acted on."""
    a64 = gt.double(actor)
    before = _obs_before(obs0, obs, K)
    out = [gt.logits64(a64, form, before[k].double()) for k in range(K)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


# ---- 1. the draws ----
@pytest.mark.parametrize("N,B", gt.SHAPES)
def test_gumbel_draws_are_the_philox_reference(N, B):
    env = _env(N, B, gt.INDEX)
    want = _draws(B, N)
    worst = 0.0
    for k in range(K):
        env._rng_offset = gt.OFFSET - 1 + k
        got = env.actor_gumbel()
        assert got.shape == (B, N, 5) and got.dtype == torch.float32
        err = np.abs(_np(got).astype(np.float64) - want[k]) / gt.gamma(want[k])
        worst = max(worst, float(err.max()))
        # the C entry itself, into a caller's buffer, at the same offset
        p = env.world.native_params(seed=gt.SEED, rng_offset=env._launch_rng_offset())
        p.env_index_base = gt.BASE
        own = torch.full((B, N, 5), 99.0, device=DEV)
        _native.check(_native.load().fg_actor_gumbel(p, B, N, own.data_ptr(), _native.current_stream(DEV)))
        assert torch.equal(own, got)
    print("%dx%d: max |g32 - g64| / gamma = %.3f" % (N, B, worst))
    assert worst <= 1.0
    assert float(want.min()) >= gt.G_MIN and float(want.max()) <= gt.G_MAX


# ---- 2. fg_actor_gumbel_pick alone ----
def _standalone(mode, explore, lg, g):
    t_lg, t_g = torch.as_tensor(lg).to(DEV), torch.as_tensor(g).to(DEV)
    n = len(lg)
    idx = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    act = torch.full((n, 2), 9.0, device=DEV)
    _native.check(_native.load().fg_actor_gumbel_pick(mode, explore, n, t_lg.data_ptr(), t_g.data_ptr() if explore else None,
                                                      idx.data_ptr(), act.data_ptr(), _native.current_stream(DEV)))
    torch.cuda.synchronize()
    return _np(idx).astype(np.int64), _np(act).astype(np.float64)


@pytest.mark.parametrize("mode", (gt.ONEHOT5, gt.INDEX))
def test_standalone_pick_and_decode(mode):
    lg, g = gt.standalone_inputs()
    l64, g64 = lg.astype(np.float64), g.astype(np.float64)
    rows = np.arange(len(lg))
    tied = (rows % 64 == 2) | (rows % 64 == 3)
    for explore in (1, 0):
        idx, act = _standalone(mode, explore, lg, g)
        want, margin = gt.pick(l64, g64, bool(explore))
        # the inputs are the kernel's own fp32 values: beta = 0, and the draws' bound stays in the band as the issue states it
        band = 2.0 * gt.gamma(g64).max(-1) + gt.SUM_ROUNDING if explore else 0.0
        keep = (margin > band) | tied                      # exact ties stay exact in fp32: the lowest index, no exemption
        assert float(keep.mean()) > 0.98 and np.array_equal(idx[keep], want[keep])
        assert int(idx.min()) >= 0 and int(idx.max()) <= 4 and np.array_equal(act, gt.decode(mode, idx))
        assert bool((idx[rows % 64 == 2] == 1).all()) and bool((idx[rows % 64 == 3] == 0).all())    # ties of two and three
        assert bool((idx[rows % 64 == 1] == 3).all()) and bool((idx[rows % 64 == 4] != 2).all())    # a logit at +/-100
        if not explore:
            assert np.array_equal(idx, want)
        print("standalone mode %d explore %d: %d of %d rows inside the band" % (mode, explore, int((~keep).sum()), len(keep)))


# ---- 3., 4. the fused launch against the fp64 actor, its replay ----
def _check_replay(env, snap, res, mode):
    obs, rew, done, info = res
    after = _state(env)
    idx = info["actions"]
    assert idx.dtype == torch.int32 and tuple(idx.shape) == tuple(done.shape) and tuple(info["u"].shape) == tuple(idx.shape) + (2,)
    src = idx.contiguous() if mode == gt.INDEX else torch.nn.functional.one_hot(idx.long(), 5).float().contiguous()
    env._restore(snap)
    r_obs, r_rew, r_done, r_info = env.rollout(src, out=False)
    assert torch.equal(obs, r_obs) and torch.equal(rew, r_rew) and torch.equal(done, r_done)
    assert torch.equal(info["individual_reward"], r_info["individual_reward"])
    for a, b in zip(after, _state(env)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("form,N,B,H,mode", gt.CASES)
def test_fused_against_fp64_and_replay(form, N, B, H, mode):
    env = _env(N, B, mode)
    actor = gt.gumbel_actor(form, N, H, device=DEV)
    assert env.actor_path(actor) == "fused"
    snap, obs0 = env._snapshot(), _current_obs(env)
    g = _draws(B, N)
    seen = set()
    for explore in (True, False):
        actor.explore = explore
        env._restore(snap)
        res = _rollout(env, actor)
        obs, rew, done, info = res
        assert "log_prob" not in info
        assert bool(done[1].all()) and not bool(done[0].any()) and not bool(done[2].any())     # the episode ends inside the launch
        lg, beta = _reference(actor, form, obs0, obs, B, N)
        assert float(np.abs(lg).max()) + gt.G_MAX < gt.Y_MAX
        want, margin = gt.pick(lg, g, explore)
        ex = gt.exempt(margin, beta, g, explore)
        idx = _np(info["actions"]).astype(np.int64)
        share = float(ex.mean())
        print("%s %dx%d H=%d mode %d explore %d: exempt share %.4f" % (form, N, B, H, mode, explore, share))
        assert share <= gt.EXEMPT_CAP, "exempt share %.4f" % share
        assert np.array_equal(idx[~ex], want[~ex]), "%d of %d rows differ" % (int((idx != want)[~ex].sum()), int((~ex).sum()))
        assert int(idx.min()) >= 0 and int(idx.max()) <= 4
        assert np.array_equal(_np(info["u"]).astype(np.float64), gt.decode(mode, idx))         # every row, exempt ones included
        seen |= set(np.unique(idx).tolist())
        _check_replay(env, snap, res, mode)                                                     # 4. the replay
        if explore:
            env._restore(snap)
            again = _rollout(env, actor)                                                        # two launches, one snapshot
            assert torch.equal(again[3]["actions"], info["actions"]) and torch.equal(again[0], obs) and torch.equal(again[1], rew)
            env._restore(snap)
            parts = [_rollout(env, actor, 1) for _ in range(K)]                                 # K = 3 equals three K = 1
            for key in ("actions", "u"):
                assert torch.equal(torch.cat([p[3][key] for p in parts]), info[key]), key
            assert torch.equal(torch.cat([p[0] for p in parts]), obs) and torch.equal(torch.cat([p[2] for p in parts]), done)
            assert torch.equal(torch.cat([p[1] for p in parts]), rew)
    assert seen == {0, 1, 2, 3, 4}


# ---- 5. N identical per-agent members give the shared kernel's bits ----
@pytest.mark.parametrize("bn", (False, True))
@pytest.mark.parametrize("N,B,H,mode", [(3, 70, 64, gt.ONEHOT5), (9, 20, 32, gt.INDEX), (27, 11, 64, gt.ONEHOT5), (32, 9, 64, gt.INDEX)])
def test_identical_members_give_the_shared_kernels_bits(N, B, H, mode, bn):
    env = _env(N, B, mode)
    shared = gt.gumbel_actor("bn" if bn else "plain", N, H, device=DEV)
    members = gt.gumbel_actor("pa_bn" if bn else "pa", N, H, device=DEV, identical=True)
    assert env.actor_path(shared) == "fused" and env.actor_path(members) == "fused"
    snap = env._snapshot()
    for explore in (True, False):
        shared.explore = members.explore = explore
        env._restore(snap)
        one = _rollout(env, shared)
        env._restore(snap)
        many = _rollout(env, members)
        assert torch.equal(one[3]["actions"], many[3]["actions"]) and torch.equal(one[3]["u"], many[3]["u"])
        assert torch.equal(one[0], many[0]) and torch.equal(one[1], many[1]) and torch.equal(one[2], many[2])


# ---- 6. the host-paced twin ----
@pytest.mark.parametrize("form,N,B,H,mode", [("plain", 9, 20, 64, gt.ONEHOT5), ("pa_bn", 9, 20, 32, gt.INDEX)])
def test_host_paced_twin_draws_the_same_and_picks_the_same(form, N, B, H, mode):
    env = _env(N, B, mode)
    actor = gt.gumbel_actor(form, N, H, device=DEV)
    twin = GumbelSoftmaxActor(_Wrap(actor.logits))       # the same function behind a module the rule does not recognise
    assert env.actor_path(actor) == "fused" and env.actor_path(twin) == "host"
    snap, obs0 = env._snapshot(), _current_obs(env)
    g = _draws(B, N)
    for explore in (True, False):
        actor.explore = twin.explore = explore
        env._restore(snap)
        fused = _rollout(env, actor)
        env._restore(snap)
        g0 = env.actor_gumbel().clone()                  # what the host-paced step 0 draws
        host = _rollout(env, twin)
        assert "log_prob" not in host[3] and host[3]["actions"].dtype == torch.int32
        assert tuple(host[3]["actions"].shape) == (K, B, N) and tuple(host[3]["u"].shape) == (K, B, N, 2)
        assert np.array_equal(_np(host[3]["u"]).astype(np.float64), gt.decode(mode, _np(host[3]["actions"]).astype(np.int64)))
        assert bool((np.abs(_np(g0).astype(np.float64) - g[0]) <= gt.gamma(g[0])).all())       # the same draws: the reference's
        with torch.no_grad():
            own, _ = env._gumbel_pick(actor.logits(obs0), g0 if explore else None, explore)     # ... and the ones the loop used
        assert torch.equal(own, host[3]["actions"][0])
        lg, beta = _reference(actor, form, obs0, fused[0], B, N)
        margin = gt.pick(lg[0], g[0], explore)[1]
        keep = ~gt.exempt(margin, beta[0], g[0], explore, scale=2.0)                            # each path's own band
        assert float(keep.mean()) >= 1.0 - 2 * gt.EXEMPT_CAP
        assert torch.equal(fused[3]["actions"][0][torch.as_tensor(keep)], host[3]["actions"][0][torch.as_tensor(keep)])


# ---- 7. the flag and the parameters are read per call ----
@pytest.mark.parametrize("form", ("plain", "pa_bn"))
def test_explore_flag_and_weights_are_read_per_launch(form):
    N, B, H, mode = 9, 20, 64, gt.ONEHOT5
    env = _env(N, B, mode)
    actor = gt.gumbel_actor(form, N, H, device=DEV)
    snap = env._snapshot()
    want = env._rollout_shapes(K, 1, act=True, idx=True)
    out = {k: env._fresh_out(k, shp) for k, shp in want.items()}
    env._roll_launchers.clear()
    runs = []
    for explore in (True, False, True, False):
        env._restore(snap)
        actor.explore = explore
        runs.append(_clone(env.rollout_actor(K, actor, out=out))[3])
    assert len(env._roll_launchers) == 1                                                  # the flag is not in the key
    assert torch.equal(runs[0]["actions"], runs[2]["actions"]) and torch.equal(runs[1]["actions"], runs[3]["actions"])
    assert not torch.equal(runs[0]["actions"], runs[1]["actions"])
    assert runs[0]["actions"].data_ptr() != 0 and "log_prob" not in runs[0]
    # an in-place update - every head zeroed but for the bias of class 2 - is seen by the bound launcher
    heads = [m[-1] for m in (actor.logits.actors if form == "pa_bn" else [actor.logits])]
    with torch.no_grad():
        for h in heads:
            h.weight.zero_()
            h.bias.copy_(torch.tensor([0.0, 0.0, 1.0, 0.0, 0.0]))
    env._restore(snap)
    actor.explore = False
    info = env.rollout_actor(K, actor, out=out)[3]
    assert len(env._roll_launchers) == 1 and bool((info["actions"] == 2).all())
    assert np.array_equal(_np(info["u"]).astype(np.float64), gt.decode(mode, _np(info["actions"]).astype(np.int64)))


def test_other_combinations_raise():
    env = _env(3, 4, gt.INDEX)
    actor = gt.gumbel_actor("plain", 3, 32, device=DEV)
    with pytest.raises(NotImplementedError):
        env.rollout_actor(2, actor.logits)
    cont = formation_gym.make_env("formation_hd_env", False, 3, num_envs=4, device=DEV)
    cont.seed(1); cont.reset()
    with pytest.raises(ValueError):
        cont.rollout_actor(2, actor)
    sc = formation_gym.load_scenario("formation_hd_env")
    world = sc.make_world(3, num_envs=4, device=DEV)
    world.discrete_action = True
    arg = formation_gym.MultiAgentEnv(world, sc.reset_world, sc.reward, sc.observation)
    arg.seed(1); arg.reset()
    with pytest.raises(NotImplementedError):
        arg.rollout_actor(2, actor)
    assert env.obs_path(torch.float16, actor=actor) == "cast"
    res = env.rollout_actor(2, actor, out=False, obs_dtype=torch.float16)
    assert res[0].dtype == torch.float16 and res[3]["actions"].dtype == torch.int32
