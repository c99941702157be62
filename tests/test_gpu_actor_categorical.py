"""GPU tests of the categorical (discrete-action) member of the fused actor rollouts: `env.rollout_actor(K, CategoricalActor)`
in the action modes FG_ACT_ONEHOT5 and FG_ACT_INDEX (`fg_rollout_hd_actor_cat`: cat_actor_kernel, ln_cat_actor_kernel,
gru_cat_actor_kernel), its host-paced twin and the helpers `fg_actor_uniform` / `fg_actor_categorical`, against the fp64
reference of tests/actor_cat_testlib.py (semantics, exemption band and mutants: that module's docstring;
tests/test_actor_categorical_cpu.py shows that these inputs tell the mutants apart and that the reference alone keeps the exempt
share under the cap).

Inputs: env_index_base = 3, a 64-bit seed, a launch base offset of 2^32 - 2 (steps 1 and 2 of a K = 3 launch carry into the high
word), world_length = 2 with auto_reset (an episode ends inside the launch: the reset draws and the GRU masking run), and the
shapes of `ct.CASES` - 3 x 70 (a second workgroup with 6 live envs), 9 x 20 (a half-empty last pass), 27 x 11 (6.75 passes),
H = 32 and 64 for the three families, H = 128 once.

Bounds.  beta, the row's logit bound, is each family's action bound with max_j |l_j| for |a| (`ct.logits64`); a sampled index
is compared outside the band |u s - c_j| <= (4 beta + 2^-16) s, which may hold at most 2 % of a case's rows; log_prob lies within
2 beta + LOGP_BOUND max(1, |log_prob|).  LOGP_BOUND is the standalone bound of `fg_actor_categorical` against fp64 on the same
fp32 logits: 4 x the maximum measured on `ct.standalone_inputs()` (profiles/actor_categorical.md), relative to max(1, |log_prob|)
because (l_idx - m) rounds at its own magnitude (up to 200 in the edge rows).
Run with `pytest -m gpu`; `-s` prints each case's measured figures as shares of their bounds.
"""
import copy

import numpy as np
import pytest
import torch

import formation_gym
from formation_gym import _native
from tests import actor_cat_testlib as ct
from tests.actor_testlib import DEV, clone as _clone, current_obs as _current_obs, obs_before as _obs_before, state as _state

pytestmark = pytest.mark.gpu

K = ct.K
LOGP_BOUND = 4 * 2.16e-7               # 4 x the measured maximum of |logp - logp64| / max(1, |logp64|) (profiles/actor_categorical.md)
EXEMPT_CAP = 0.02
MODES = (ct.ONEHOT5, ct.INDEX)


def _env(N, B, mode, base=ct.BASE):
    sc = formation_gym.load_scenario("formation_hd_env")
    world = sc.make_world(N, num_envs=B, device=DEV)
    env = formation_gym.MultiAgentEnv(world, sc.reset_world, sc.reward, sc.observation, discrete_action=(mode == ct.ONEHOT5))
    env.discrete_action_input = mode == ct.INDEX
    env.seed(3)
    env.reset()
    env.auto_reset = True
    env.world.world_length = 2
    env.scenario._seed = ct.SEED                 # what `seed()` stores, without the host streams a 64-bit seed cannot key
    env.scenario.env_base = base
    env._rng_offset = ct.OFFSET - 1              # the next launch draws at OFFSET
    assert env._launch_rng_offset() == ct.OFFSET and env._action_mode() == mode
    return env


def _state0(fam, B, N, H, seed=7):
    if fam != "gru":
        return None
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((B, N, H), generator=g) - 0.5).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _reference(actor, fam, obs0, obs, info, greedy, B, N):
    """Per step: (idx, logp, margin, beta) of the fp64 actor on the observation (and fp32 GRU state) the step acted on."""
    a64 = copy.deepcopy(actor).double()
    u = ct.launch_uniforms(ct.SEED, ct.BASE, B, N, ct.OFFSET, K)
    before = _obs_before(obs0, obs, K)
    out = []
    for k in range(K):
        h = info["rnn_states"][k].double() if fam == "gru" else None
        lg, beta, hn, hb = ct.logits64(a64, fam, before[k].double(), h)
        idx, logp, margin = ct.pick(lg, u[k], greedy)
        out.append(dict(idx=idx, logp=logp, margin=margin, beta=beta, h=hn, hb=hb, lg=lg))
    return out


def _rollout(env, actor, fam, h0, **kw):
    h = None if h0 is None else h0.clone()
    extra = dict(rnn_state=h, rnn_states_every=1) if fam == "gru" else {}
    return _clone(env.rollout_actor(K, actor, out=False, **extra, **kw))


# ---- 1. the uniform draws ----
@pytest.mark.parametrize("N,B", ct.SHAPES)
def test_uniform_draws_are_the_philox_reference(N, B):
    env = _env(N, B, ct.INDEX)
    want = ct.launch_uniforms(ct.SEED, ct.BASE, B, N, ct.OFFSET, K)
    for k in range(K):
        env._rng_offset = ct.OFFSET - 1 + k
        got = env.actor_uniform()
        assert got.shape == (B, N) and got.dtype == torch.float32
        assert np.array_equal(_np(got).astype(np.float64), want[k]), "step %d" % k
    assert float(want.min()) >= 0.0 and float(want.max()) < 1.0


# ---- 2. fg_actor_categorical alone ----
def _standalone(mode, greedy, lg, u):
    lib = _native.load()
    t_lg, t_u = torch.as_tensor(lg).to(DEV), torch.as_tensor(u).to(DEV)
    n = len(lg)
    idx = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    act = torch.full((n, 2), 9.0, device=DEV)
    logp = torch.full((n,), 9.0, device=DEV)
    _native.check(lib.fg_actor_categorical(mode, greedy, n, t_lg.data_ptr(), t_u.data_ptr(), idx.data_ptr(), act.data_ptr(),
                                           logp.data_ptr(), _native.current_stream(DEV)))
    torch.cuda.synchronize()
    return _np(idx).astype(np.int64), _np(act).astype(np.float64), _np(logp).astype(np.float64)


@pytest.mark.parametrize("mode", MODES)
def test_standalone_pick_decode_and_log_prob(mode):
    lg, u = ct.standalone_inputs()
    l64, u64 = lg.astype(np.float64), u.astype(np.float64)
    rows = np.arange(len(lg))
    # sampled: the index of the fp64 rule outside the band eta_0 = 2^-16, the decode exact, the log-prob within the bound
    idx, act, logp = _standalone(mode, 0, lg, u)
    want, wlogp, margin = ct.pick(l64, u64)
    keep = ~ct.exempt(margin, 0.0)
    assert float(keep.mean()) > 0.7 and np.array_equal(idx[keep], want[keep])
    assert int(idx.min()) >= 0 and int(idx.max()) <= 4 and np.array_equal(act, ct.decode(mode, idx))
    assert bool((idx[(u == 0) & (rows % 64 == 0)] == 0).all())                          # u = 0, equal logits: the first class
    assert bool((idx[(u == u.max()) & (rows % 64 == 0)] == 4).all())                    # the largest u, equal logits: the last
    assert bool((idx[rows % 64 == 1] == 3).all())                                       # underflowing classes are never taken
    own = np.take_along_axis(l64 - l64.max(-1, keepdims=True), idx[:, None], 1)[:, 0] - np.log(np.exp(l64 - l64.max(-1, keepdims=True)).sum(-1))
    err = np.abs(logp - own) / np.maximum(1.0, np.abs(own))                             # against fp64 at the index it took
    print("standalone mode %d: max |logp - logp64| / max(1, |logp64|) = %.3g (%.2f of the bound), %d of %d rows exempt"
          % (mode, err.max(), err.max() / LOGP_BOUND, int((~keep).sum()), len(keep)))
    assert np.isfinite(logp).all() and float(err.max()) <= LOGP_BOUND
    # greedy: the lowest index of the maximum, ties included, with no exemptions
    gidx, gact, glogp = _standalone(mode, 1, lg, u)
    gwant, gwlogp, _ = ct.pick(l64, greedy=True)
    assert np.array_equal(gidx, gwant) and np.array_equal(gact, ct.decode(mode, gwant))
    assert bool((gidx[rows % 64 == 2] == 1).all()) and bool((gidx[rows % 64 == 0] == 0).all())
    assert float((np.abs(glogp - gwlogp) / np.maximum(1.0, np.abs(gwlogp))).max()) <= LOGP_BOUND


# ---- 3., 4., 7. the fused launch against the fp64 actor, its replay, the recurrent member ----
def _check_replay(env, snap, res, mode):
    obs, rew, done, info = res
    after = _state(env)
    idx = info["actions"]
    assert idx.dtype == torch.int32 and tuple(idx.shape) == tuple(done.shape) and tuple(info["u"].shape) == tuple(idx.shape) + (2,)
    # info['u'] is fg_decode_actions of the indices (INDEX mode's table; the one-hot through ONEHOT5's)
    B, N = idx.shape[1:]
    dec = torch.empty_like(info["u"])
    src = idx.contiguous() if mode == ct.INDEX else torch.nn.functional.one_hot(idx.long(), 5).float().contiguous()
    _native.check(_native.load().fg_decode_actions(mode, idx.numel(), src.data_ptr(), dec.data_ptr(), _native.current_stream(DEV)))
    assert torch.equal(dec, info["u"])
    env._restore(snap)
    r_obs, r_rew, r_done, r_info = env.rollout(src, out=False)
    assert torch.equal(obs, r_obs) and torch.equal(rew, r_rew) and torch.equal(done, r_done)
    assert torch.equal(info["individual_reward"], r_info["individual_reward"])
    for a, b in zip(after, _state(env)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fam,N,B,H", ct.CASES)
def test_fused_sampled_against_fp64_and_replay(fam, N, B, H, mode):
    env = _env(N, B, mode)
    actor = ct.cat_actor(fam, N, H, seed=ct.case_seed(fam, N, B, H), device=DEV)
    assert env.actor_path(actor) == "fused"
    h0 = _state0(fam, B, N, H)
    snap, obs0 = env._snapshot(), _current_obs(env)
    res = _rollout(env, actor, fam, h0)
    obs, rew, done, info = res
    assert bool(done[1].all()) and not bool(done[0].any()) and not bool(done[2].any())     # the episode ends inside the launch
    ref = _reference(actor, fam, obs0, obs, info, False, B, N)
    idx, logp = _np(info["actions"]).astype(np.int64), _np(info["log_prob"]).astype(np.float64)
    ex = np.stack([ct.exempt(r["margin"], r["beta"]) for r in ref])
    want = np.stack([r["idx"] for r in ref])
    share = float(ex.mean())
    assert share <= EXEMPT_CAP, "exempt share %.4f" % share
    assert np.array_equal(idx[~ex], want[~ex]), "%d of %d rows differ" % (int((idx != want)[~ex].sum()), int((~ex).sum()))
    assert int(idx.min()) >= 0 and int(idx.max()) <= 4
    assert np.array_equal(_np(info["u"]).astype(np.float64), ct.decode(mode, idx))
    # log_prob at the index the kernel took, against fp64 on the same observation
    worst = 0.0
    for k in range(K):
        lsm = ref[k]["lg"] - ref[k]["lg"].max(-1, keepdims=True)
        own = np.take_along_axis(lsm, idx[k][..., None], -1)[..., 0] - np.log(np.exp(lsm).sum(-1))
        bound = 2.0 * ref[k]["beta"] + LOGP_BOUND * np.maximum(1.0, np.abs(own))
        worst = max(worst, float((np.abs(logp[k] - own) / bound).max()))
    print("%s %dx%d H=%d mode %d: exempt %.4f, log_prob err / bound %.3g" % (fam, N, B, H, mode, share, worst))
    assert worst <= 1.0
    if fam == "gru":                                     # 7. the recurrent member
        states = info["rnn_states"]
        assert tuple(states.shape) == (K, B, N, H) and torch.equal(states[0], h0)
        assert not bool(states[2].any()) and bool(states[1].any())                    # zeroed where step 1 ended the episode
        _check_states(ref, info, done)
    _check_replay(env, snap, res, mode)


def _check_states(ref, info, done):
    """Every kept state and the state left behind against the fp64 step on the state the step acted with, masked by the step's
    done flags, within the recurrent state bound of each row, TOL max(1, r1) max(1, r2) (tests/actor_fidelity.py rec_bounds);
    finished rows hold exactly 0."""
    after = [info["rnn_states"][k + 1] for k in range(K - 1)] + [info["rnn_state"]]
    for k in range(K):
        live = (~done[k]).unsqueeze(-1)
        assert not bool(after[k][done[k]].any())
        err = ((after[k].double() - ref[k]["h"]).abs() * live.double())
        assert bool((err <= ref[k]["hb"]).all()), (k, float((err / ref[k]["hb"]).max()))


# (family, N, B, H, eps of the LayerNorms): every case at the builders' NORM_EPS, and - greedy needs no band - the two
# LayerNorm families at the trainers' default eps = 1e-5 as well, where the rstd factors are the kernels' everyday ones
GREEDY_CASES = [c + (None,) for c in ct.CASES] + [(fam, n, b, 64, 1e-5) for fam in ("ln", "gru") for (n, b) in ct.SHAPES]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fam,N,B,H,eps", GREEDY_CASES)
def test_fused_greedy_equals_the_fp64_mode_without_exemptions(fam, N, B, H, eps, mode):
    env = _env(N, B, mode)
    h0 = _state0(fam, B, N, H)
    snap, obs0 = env._snapshot(), _current_obs(env)
    for seed in range(12):                               # inputs whose fp64 top-two gap exceeds 2 beta in every row
        actor = ct.cat_actor(fam, N, H, seed=seed, device=DEV, deterministic=True, norm_eps=eps)
        env._restore(snap)
        obs, rew, done, info = _rollout(env, actor, fam, h0)
        ref = _reference(actor, fam, obs0, obs, info, True, B, N)
        if all(bool((r["margin"] > 2.0 * r["beta"]).all()) for r in ref):
            break
    else:
        pytest.fail("no actor seed whose reference rows all have a top-two gap above 2 beta")
    idx = _np(info["actions"]).astype(np.int64)
    want = np.stack([r["idx"] for r in ref])
    assert np.array_equal(idx, want)
    logp = _np(info["log_prob"]).astype(np.float64)
    wlogp, beta = np.stack([r["logp"] for r in ref]), np.stack([r["beta"] for r in ref])
    assert bool((np.abs(logp - wlogp) <= 2.0 * beta + LOGP_BOUND * np.maximum(1.0, np.abs(wlogp))).all())
    assert np.array_equal(_np(info["u"]).astype(np.float64), ct.decode(mode, idx))
    if fam == "gru":
        _check_states(ref, info, done)
    _check_replay(env, snap, (obs, rew, done, info), mode)


# ---- 5. fused = host-paced, and a two-shard split ----
def _all_outside(ref):
    return not any(bool(ct.exempt(r["margin"], r["beta"]).any()) for r in ref)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("fam,N,B,H", [("plain", 27, 11, 64), ("ln", 9, 20, 32), ("gru", 3, 70, 64)])
def test_fused_equals_host_paced_and_shards(fam, N, B, H, mode):
    env = _env(N, B, mode)
    h0 = _state0(fam, B, N, H)
    snap, obs0 = env._snapshot(), _current_obs(env)
    start = _state(env)
    for seed in range(6):                                # a case whose reference rows are all outside the exemption band
        actor = ct.cat_actor(fam, N, H, seed=seed, device=DEV)
        env._restore(snap)
        fused = _rollout(env, actor, fam, h0)
        if _all_outside(_reference(actor, fam, obs0, fused[0], fused[3], False, B, N)):
            break
    else:
        pytest.fail("no actor seed whose reference rows are all outside the exemption band")
    env._restore(snap)
    draws = []
    for k in range(K):
        env._rng_offset = ct.OFFSET - 1 + k
        draws.append(env.actor_uniform().clone())
    env._restore(snap)
    env.post_step_callback = lambda world: None          # a callback: the host-paced loop
    assert env.actor_path(actor) == "host"
    host = _rollout(env, actor, fam, h0)
    env.post_step_callback = None
    assert torch.equal(fused[3]["actions"], host[3]["actions"]) and torch.equal(fused[3]["u"], host[3]["u"])
    assert host[3]["actions"].dtype == torch.int32
    assert torch.equal(fused[0], host[0]) and torch.equal(fused[1], host[1]) and torch.equal(fused[2], host[2])
    ref = _reference(actor, fam, obs0, fused[0], fused[3], False, B, N)
    beta, wlogp = np.stack([r["beta"] for r in ref]), np.stack([r["logp"] for r in ref])
    gap = np.abs(_np(fused[3]["log_prob"]).astype(np.float64) - _np(host[3]["log_prob"]).astype(np.float64))
    assert bool((gap <= 4.0 * beta + 2.0 * LOGP_BOUND * np.maximum(1.0, np.abs(wlogp))).all())    # each path's own bound
    # the draws of both paths are the reference's: the same u at every step
    want_u = ct.launch_uniforms(ct.SEED, ct.BASE, B, N, ct.OFFSET, K)
    assert np.array_equal(np.stack([_np(d) for d in draws]).astype(np.float64), want_u)
    # two shards with env_index_base give the full batch's slices
    cut = B // 2 + 1
    for lo, hi in ((0, cut), (cut, B)):
        shard = _env(N, hi - lo, mode, base=ct.BASE + lo)
        w, sc = shard.world, shard.scenario
        for dst, src in zip((w.pos_x, w.pos_y, w.vel_x, w.vel_y, w.step_count, sc.ideal_shape, sc.ideal_vel), start):
            dst.copy_(src[lo:hi])
        sc._cache = None
        part = _rollout(shard, actor, fam, None if h0 is None else h0[lo:hi])
        assert torch.equal(part[3]["actions"], fused[3]["actions"][:, lo:hi]) and torch.equal(part[0], fused[0][:, lo:hi])
        assert torch.equal(part[3]["log_prob"], fused[3]["log_prob"][:, lo:hi]) and torch.equal(part[1], fused[1][:, lo:hi])


# ---- 6. splitting K; the greedy flag is read per launch ----
@pytest.mark.parametrize("mode", MODES)
def test_split_k_and_the_flag_per_launch(mode):
    fam, N, B, H = "gru", 9, 20, 32
    env = _env(N, B, mode)
    actor = ct.cat_actor(fam, N, H, device=DEV)
    h0 = _state0(fam, B, N, H)
    snap = env._snapshot()
    h = h0.clone()
    whole = _clone(env.rollout_actor(K, actor, out=False, rnn_state=h, rnn_states_every=2))
    assert whole[3]["rnn_state"] is not None and tuple(whole[3]["rnn_states"].shape) == (2, B, N, H)
    assert torch.equal(whole[3]["rnn_states"][0], h0)
    env._restore(snap)
    h1 = h0.clone()
    parts = [_clone(env.rollout_actor(1, actor, out=False, rnn_state=h1, rnn_states_every=2)) for _ in range(K)]
    assert torch.equal(h1, h)                                                             # in place, step by step
    for key in ("actions", "u", "log_prob"):
        assert torch.equal(torch.cat([p[3][key] for p in parts]), whole[3][key]), key
    assert torch.equal(torch.cat([p[0] for p in parts]), whole[0]) and torch.equal(torch.cat([p[2] for p in parts]), whole[2])
    assert torch.equal(parts[2][3]["rnn_states"][0], whole[3]["rnn_states"][1])           # the state step 2 acted with
    # one bound launcher, greedy and sampled calls alternating
    want = env._rollout_shapes(K, 1, act=True, log_prob=True, idx=True)
    out = {k: env._fresh_out(k, shp) for k, shp in want.items()}
    runs, hs = [], h0.clone()
    env._roll_launchers.clear()
    for det in (False, True, False, True):
        env._restore(snap)
        actor.deterministic = det
        hs.copy_(h0)
        runs.append(_clone(env.rollout_actor(K, actor, out=out, rnn_state=hs))[3])
    assert len(env._roll_launchers) == 1                                                  # the flag is not in the key
    assert torch.equal(runs[0]["actions"], runs[2]["actions"]) and torch.equal(runs[1]["actions"], runs[3]["actions"])
    assert torch.equal(runs[0]["actions"], whole[3]["actions"]) and not torch.equal(runs[0]["actions"], runs[1]["actions"])
    assert torch.equal(runs[0]["log_prob"], whole[3]["log_prob"])


def test_default_buffers_are_placed_in_a_discrete_mode():
    """out=None at a shape whose observation buffer is large enough for the placement probe (286 MB): the probe's own launches
    take continuous actions, the env stays in its mode, and the placed launch gives the bits of a launch into fresh buffers."""
    N, B, Kp = 27, 4096, 4
    env = _env(N, B, ct.INDEX)
    actor = ct.cat_actor("plain", N, 32, device=DEV)
    snap = env._snapshot()
    fresh = _clone(env.rollout_actor(Kp, actor, out=False))
    env._restore(snap)
    placed = env.rollout_actor(Kp, actor)
    assert env.placement.get("probed") and env._action_mode() == ct.INDEX
    assert torch.equal(placed[3]["actions"], fresh[3]["actions"]) and torch.equal(placed[0], fresh[0])
    assert torch.equal(placed[3]["log_prob"], fresh[3]["log_prob"]) and torch.equal(placed[3]["u"], fresh[3]["u"])
    again = env.rollout_actor(Kp, actor)                 # the env's own buffers, bound once
    assert again[3]["actions"].data_ptr() == placed[3]["actions"].data_ptr()


def test_other_combinations_raise():
    env = _env(3, 4, ct.INDEX)
    plain = ct.cat_actor("plain", 3, 32, device=DEV)
    with pytest.raises(NotImplementedError):
        env.rollout_actor(2, plain.logits)
    cont = formation_gym.make_env("formation_hd_env", False, 3, num_envs=4, device=DEV)
    cont.seed(1); cont.reset()
    with pytest.raises(ValueError):
        cont.rollout_actor(2, plain)
    sc = formation_gym.load_scenario("formation_hd_env")
    world = sc.make_world(3, num_envs=4, device=DEV)
    world.discrete_action = True
    arg = formation_gym.MultiAgentEnv(world, sc.reset_world, sc.reward, sc.observation)
    arg.seed(1); arg.reset()
    with pytest.raises(NotImplementedError):
        arg.rollout_actor(2, plain)
