"""16-bit observations out of the fused actor launch (`rollout_actor(..., obs_dtype=)`): the launches `fg_rollout_hd_actor_obs16`
and `fg_rollout_hd_actor_cat_obs16` against the fp32 `rollout_actor` call cast by torch, bit for bit, and the 'cast' route behind
the same argument.

The method is tests/test_gpu_obs16.py's: there is no tolerance anywhere in this file.  A 16-bit observation is DEFINED as
`.to(dtype)` of the fp32 call's value (round to nearest even, fp16 overflow to inf, fp16 subnormals and signed zeros kept), the
16-bit writer does the fp32 writer's subtractions on the same table entries, and everything but the observations is the fp32
call's, so every comparison is `torch.equal` - on the raw 16-bit patterns for the observations.  The fp32 reference holds no NaN
for these inputs (asserted), so NaN payloads never enter a comparison and no element is left out.

Shapes: the smallest batch at which each geometry (E envs per workgroup, four writer waves) has a full workgroup and a ragged
one with a partly filled wave tile - 3 agents x 102 envs (E = 64: the second workgroup's waves hold 16, 16, 6 and 0 envs),
9 x 23 (E = 16: 4, 3, 0, 0) and 27 x 13 (E = 8: two envs for wave 0, one for the others).  Env blocks of 27 / 243 / 2187 words
put consecutive envs at all four 16-byte phases.  K = 5 with episode_length = 3 puts an auto-reset - and the GRU state's masking -
inside the launch."""
import numpy as np
import pytest
import torch

import formation_gym
from formation_gym import GaussianActor
from tests import actor_cat_testlib as ct
from tests import actor_testlib as at
from tests.test_gpu_obs16 import PLANTED, _classes

pytestmark = pytest.mark.gpu

DEV = at.DEV
K = 5
ENVS = {3: 102, 9: 23, 27: 13}
DTYPES = [torch.float16, torch.bfloat16]
KINDS = ("gauss", "cat")
FAMILIES = ("plain", "ln", "gru")


def _env(N, B, discrete=False, name="formation_hd_env", auto_reset=True, seed=3):
    sc = formation_gym.load_scenario(name)
    kw = dict(episode_length=3) if name == "formation_hd_env" else {}                  # (the landmark scenarios take none)
    world = sc.make_world(N, num_envs=B, device=DEV, **kw)
    e = formation_gym.MultiAgentEnv(world, sc.reset_world, sc.reward, sc.observation, discrete_action=discrete)
    e.seed(seed)
    e.reset()
    e.auto_reset = auto_reset
    return e


def _actor(kind, fam, N, H, seed=0):
    """The Gaussian or the categorical member of the family: actor_cat_testlib's body under a head of two means or five logits."""
    if kind == "cat":
        return ct.cat_actor(fam, N, H, seed=seed, device=DEV)
    mean = ct.cat_actor(fam, N, H, seed=seed, head=2).logits
    return GaussianActor(mean, torch.nn.Parameter(torch.tensor([-0.7, -1.1]))).to(DEV)


def _rnn_state(fam, B, N, H, seed=7):
    if fam != "gru":
        return None
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((B, N, H), generator=g) - 0.5).to(DEV)


def _state(e):
    w, sc = e.world, e.scenario
    st = [w.pos_x, w.pos_y, w.vel_x, w.vel_y, w.step_count]
    st += [getattr(sc, k) for k in ("ideal_shape", "ideal_vel") if torch.is_tensor(getattr(sc, k, None))]
    return [t.clone() for t in st] + [torch.tensor(e._rng_offset)]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _run(e, snap, call):
    """`call()` from the snapshot: (obs, reward, done, info tensors by key, the state left behind)."""
    e._restore(snap)
    obs, rew, done, info = call()
    torch.cuda.synchronize()
    return obs, rew, done, info, _state(e)


def _call(e, actor, h0, K_=K, **kw):
    """`rollout_actor` with a fresh copy of the initial hidden state (the call updates it in place)."""
    def call():
        state = {} if h0 is None else dict(rnn_state=h0.clone(), rnn_states_every=2)
        return e.rollout_actor(K_, actor, **dict(state, **kw))
    return call


def _assert_same_but_obs(ref, got, dtype):
    obs32, rew32, done32, info32, st32 = ref
    obs16, rew16, done16, info16, st16 = got
    assert not torch.isnan(obs32).any()
    assert obs16.dtype == dtype and obs16.shape == obs32.shape and obs16.is_contiguous()
    assert torch.equal(_bits(obs16), _bits(obs32.to(dtype)))
    assert torch.equal(rew16, rew32) and torch.equal(done16, done32)
    assert sorted(info16) == sorted(info32)
    for k in info32:
        assert info16[k].dtype == info32[k].dtype and torch.equal(info16[k], info32[k]), k
    for a, b in zip(st16, st32):
        assert torch.equal(a, b)


def _check_bits(kind, fam, N, H, obs_every=1):
    B = ENVS[N]
    e = _env(N, B, discrete=kind == "cat")
    actor = _actor(kind, fam, N, H)
    h0 = _rnn_state(fam, B, N, H)
    snap = e._snapshot()
    ref = _run(e, snap, _call(e, actor, h0, out=False, obs_every=obs_every))
    assert ref[2].any() and not ref[2].all()               # the episode boundary is inside the launch
    assert ref[0].shape == (K // obs_every, B, N, 6 * N)
    want = {"actions", "log_prob", "individual_reward"} | ({"u"} if kind == "cat" else set()) \
        | ({"rnn_state", "rnn_states"} if fam == "gru" else set())
    assert set(ref[3]) == want
    for dtype in DTYPES:
        assert e.actor_path(actor) == "fused" and e.obs_path(dtype, actor=actor) == "fused"
        got = _run(e, snap, _call(e, actor, h0, out=False, obs_every=obs_every, obs_dtype=dtype))
        _assert_same_but_obs(ref, got, dtype)


@pytest.mark.parametrize("H", [32, 64])
@pytest.mark.parametrize("N", sorted(ENVS))
@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("kind", KINDS)
def test_bits(kind, fam, N, H):
    _check_bits(kind, fam, N, H)


@pytest.mark.parametrize("N", sorted(ENVS))
def test_bits_every_second_step(N):
    _check_bits("gauss", "ln", N, 64, obs_every=2)


def test_rounding_classes():
    N, B = 9, ENVS[9]
    e = _env(N, B, auto_reset=False)                       # no reset: the planted formation stays for all K steps
    shape = np.stack([np.roll(PLANTED, b) for b in range(B)]).reshape(B, N, 2)
    ivel = np.stack([np.roll(PLANTED, 3 * b + 1)[:2] for b in range(B)])
    e.scenario.set_formation(e.world, shape, ivel)
    assert np.array_equal(e.scenario.ideal_shape.cpu().numpy().view(np.uint32), shape.view(np.uint32))
    actor = _actor("gauss", "ln", N, 32)
    snap = e._snapshot()
    ref = _run(e, snap, _call(e, actor, None, out=False))
    missing = [k for k, v in _classes(ref[0]).items() if not v]
    assert not missing, missing
    got = {}
    for dtype in DTYPES:
        assert e.obs_path(dtype, actor=actor) == "fused"
        got[dtype] = _run(e, snap, _call(e, actor, None, out=False, obs_dtype=dtype))
        _assert_same_but_obs(ref, got[dtype], dtype)
    assert torch.isinf(got[torch.float16][0]).any() and torch.isfinite(got[torch.bfloat16][0]).all()      # 65520


# ---- the 'cast' route, and a caller's `out`
def _out(e, dtype, K_=K, pad=0, log_prob=False):
    B, N = e.num_envs, e.num_agents
    D = e._out["obs"].shape[-1]
    f = dict(dtype=torch.float32, device=DEV)
    if pad:
        obs = torch.zeros((K_, B, N * D + pad), dtype=dtype, device=DEV)[:, :, :N * D].unflatten(-1, (N, D))
        assert not obs.is_contiguous()
    else:
        obs = torch.zeros((K_, B, N, D), dtype=dtype, device=DEV)
    out = dict(obs=obs, reward=torch.empty((K_, B, N), **f), indiv=torch.empty((K_, B, N), **f),
               done=torch.zeros((K_, B, N), dtype=torch.uint8, device=DEV), act=torch.empty((K_, B, N, 2), **f))
    if log_prob:
        out["log_prob"] = torch.empty((K_, B, N), **f)
    return out


def _cast_case(which):
    """(env, actor, whether the fp32 call is a fused launch that fills a caller's `out` itself, whether it returns log-probs)"""
    if which == "deterministic":
        return _env(9, 7), at.scaled_mlp(54, 32, True), True, False
    if which == "four agents":
        return _env(4, 5), _actor("gauss", "ln", 4, 32), True, True
    if which == "host-paced":
        return _env(9, 7), at.Wrap(at.scaled_mlp(54, 32, True)), False, False
    e = _env(3, 5, name="basic_formation_env")
    mlp = at.scaled_mlp(e._out["obs"].shape[-1], 32, True)
    return e, mlp, e.actor_path(mlp) == "fused", False


@pytest.mark.parametrize("which", ["deterministic", "four agents", "host-paced", "basic_formation_env"])
def test_cast_route_and_callers_out(which):
    e, actor, launches, log_prob = _cast_case(which)
    assert (e.actor_path(actor) == "fused") == launches
    snap = e._snapshot()
    ref = _run(e, snap, _call(e, actor, None, out=False))
    for dtype in DTYPES:
        assert e.obs_path(dtype, actor=actor) == "cast"
        got = _run(e, snap, _call(e, actor, None, out=False, obs_dtype=dtype))
        _assert_same_but_obs(ref, got, dtype)
        again = _run(e, snap, _call(e, actor, None, obs_dtype=dtype))                   # out=None: fresh tensors as well
        _assert_same_but_obs(ref, again, dtype)
        assert again[0].data_ptr() != got[0].data_ptr()
        out = _out(e, dtype, log_prob=log_prob)
        mine = _run(e, snap, _call(e, actor, None, out=out, obs_dtype=dtype))
        assert mine[0] is out["obs"]
        _assert_same_but_obs(ref, mine, dtype)
        if launches:                                       # filled in place (a host-paced loop returns its own tensors)
            assert torch.equal(out["indiv"], ref[3]["individual_reward"]) and torch.equal(out["done"].view(torch.bool), ref[2])
            assert torch.equal(out["act"], ref[3]["actions"])
        e._restore(snap)
        with pytest.raises(ValueError):
            e.rollout_actor(K, actor, out=_out(e, dtype, pad=16, log_prob=log_prob), obs_dtype=dtype)    # a padded env pitch
        with pytest.raises(ValueError):
            e.rollout_actor(K, actor, out=_out(e, torch.float32, log_prob=log_prob), obs_dtype=dtype)    # another dtype
    with pytest.raises(ValueError):
        e.rollout_actor(K, actor, out=False, obs_dtype=torch.float64)


def test_fused_route_into_a_callers_out_and_a_single_step():
    N, B = 9, ENVS[9]
    e = _env(N, B)
    actor = _actor("gauss", "ln", N, 64)
    snap = e._snapshot()
    ref = _run(e, snap, _call(e, actor, None, out=False))
    one = _run(e, snap, _call(e, actor, None, K_=1, out=False))
    for dtype in DTYPES:
        assert e.obs_path(dtype, actor=actor) == "fused"
        out = _out(e, dtype, log_prob=True)
        for _ in range(2):                                 # the second call takes the bound launch
            mine = _run(e, snap, _call(e, actor, None, out=out, obs_dtype=dtype))
            assert mine[0] is out["obs"] and mine[3]["log_prob"] is out["log_prob"]
            _assert_same_but_obs(ref, mine, dtype)
        assert torch.equal(out["indiv"], ref[3]["individual_reward"]) and torch.equal(out["act"], ref[3]["actions"])
        e._restore(snap)
        with pytest.raises(ValueError):
            e.rollout_actor(K, actor, out=_out(e, dtype, pad=16, log_prob=True), obs_dtype=dtype)
        with pytest.raises(ValueError):
            e.rollout_actor(K, actor, out=_out(e, torch.float32, log_prob=True), obs_dtype=dtype)
        _assert_same_but_obs(one, _run(e, snap, _call(e, actor, None, K_=1, out=False, obs_dtype=dtype)), dtype)   # K = 1: fused
    with pytest.raises(ValueError):
        e.rollout_actor(K, actor, out=False, obs_dtype=torch.float64)


@pytest.mark.parametrize("kind,fam,N", [("gauss", "plain", 3), ("cat", "ln", 9), ("gauss", "gru", 27)])
def test_two_launches_give_the_same_bits(kind, fam, N):
    B = ENVS[N]
    e = _env(N, B, discrete=kind == "cat")
    actor = _actor(kind, fam, N, 64)
    h0 = _rnn_state(fam, B, N, 64)
    snap = e._snapshot()
    for dtype in DTYPES:
        a = _run(e, snap, _call(e, actor, h0, out=False, obs_dtype=dtype))
        b = _run(e, snap, _call(e, actor, h0, out=False, obs_dtype=dtype))
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1])
        assert torch.equal(a[3]["actions"], b[3]["actions"]) and torch.equal(a[3]["log_prob"], b[3]["log_prob"])


def test_a_launch_equals_its_split():
    """K = 5 against 2 + 3 steps that pass rnn_state along: the observation bits concatenated, and the final state."""
    N, B, H = 9, ENVS[9], 64
    e = _env(N, B)
    actor = _actor("gauss", "gru", N, H)
    h0 = _rnn_state("gru", B, N, H)
    snap = e._snapshot()
    for dtype in DTYPES:
        e._restore(snap)
        h = h0.clone()
        whole = e.rollout_actor(K, actor, out=False, rnn_state=h, obs_dtype=dtype)
        whole_state, whole_h = _state(e), h.clone()
        e._restore(snap)
        h = h0.clone()
        first = e.rollout_actor(2, actor, out=False, rnn_state=h, obs_dtype=dtype)
        second = e.rollout_actor(3, actor, out=False, rnn_state=h, obs_dtype=dtype)
        assert first[3]["rnn_state"] is h and second[3]["rnn_state"] is h
        assert torch.equal(_bits(whole[0]), _bits(torch.cat([first[0], second[0]])))
        assert torch.equal(whole[1], torch.cat([first[1], second[1]])) and torch.equal(whole[2], torch.cat([first[2], second[2]]))
        assert torch.equal(whole[3]["log_prob"], torch.cat([first[3]["log_prob"], second[3]["log_prob"]]))
        assert torch.equal(whole_h, h)
        for a, b in zip(whole_state, _state(e)):
            assert torch.equal(a, b)
