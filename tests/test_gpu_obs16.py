"""16-bit observations out of the rollout launch (`rollout(..., obs_dtype=)`, `rollout_policy(..., obs_dtype=)`): the fused
launches (`fg_rollout_hd_obs16`, `fg_rollout_hd_policy_obs16`) against the fp32 launch cast by torch, bit for bit, and the 'cast'
route behind the same argument.

There is no tolerance anywhere in this file: a 16-bit observation is DEFINED as `.to(dtype)` of the fp32 launch's value (round
to nearest even, fp16 overflow to inf, fp16 subnormals and signed zeros kept), the writer does the fp32 writers' subtractions on
the same operands, and so every comparison is `torch.equal` on the raw 16-bit patterns.  The fp32 reference holds no NaN for
these inputs (asserted), so NaN payloads never enter a comparison and no element is left out.

Shapes: the smallest batch at which each kernel has a full and a partial workgroup (E envs per workgroup) - 27 agents x 21 envs
(E = 16), 9 x 7 (E = 4), 3 x 19 (E = 16).  K = 5 crosses the four-step action batches of the 27-agent kernel and ends on an odd
step; episode_length = 3 puts a device auto-reset inside the launch."""
import numpy as np
import pytest
import torch

import formation_gym

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K = 5
SHAPES = [(27, 21), (9, 7), (3, 19)]
DTYPES = [torch.float16, torch.bfloat16]


def _env(N, B, name="formation_hd_env", auto_reset=True, seed=3):
    kw = dict(episode_length=3) if name == "formation_hd_env" else {}                  # (the landmark scenarios take none)
    e = formation_gym.make_env(name, False, N, num_envs=B, device=DEV, **kw)
    e.seed(seed)
    e.reset()
    e.auto_reset = auto_reset
    return e


def _actions(e, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((K, e.num_envs, e.num_agents, 2), generator=g) * 2 - 1).to(DEV)


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


def _assert_same_but_obs(ref, got, dtype):
    obs32, rew32, done32, info32, st32 = ref
    obs16, rew16, done16, info16, st16 = got
    assert not torch.isnan(obs32).any()
    assert obs16.dtype == dtype and obs16.shape == obs32.shape and obs16.is_contiguous()
    assert torch.equal(_bits(obs16), _bits(obs32.to(dtype)))
    assert torch.equal(rew16, rew32) and torch.equal(done16, done32)
    assert sorted(info16) == sorted(info32)
    for k in info32:
        assert torch.equal(info16[k], info32[k]), k
    for a, b in zip(st16, st32):
        assert torch.equal(a, b)


@pytest.mark.parametrize("obs_every", [1, 2])
@pytest.mark.parametrize("N,B", SHAPES)
def test_open_loop_bits(N, B, obs_every):
    e = _env(N, B)
    acts = _actions(e)
    snap = e._snapshot()
    ref = _run(e, snap, lambda: e.rollout(acts, out=False, obs_every=obs_every))
    assert ref[2].any() and not ref[2].all()               # the episode boundary is inside the launch
    assert ref[0].shape == (K // obs_every, B, N, 6 * N)
    for dtype in DTYPES:
        assert e.obs_path(dtype) == "fused"
        got = _run(e, snap, lambda: e.rollout(acts, out=False, obs_every=obs_every, obs_dtype=dtype))
        _assert_same_but_obs(ref, got, dtype)


@pytest.mark.parametrize("N,B", SHAPES[:2])
def test_closed_loop_bits(N, B):
    e = _env(N, B)
    snap = e._snapshot()
    ref = _run(e, snap, lambda: e.rollout_policy(K, 3, out=False))
    assert "actions" in ref[3] and ref[2].any()
    for dtype in DTYPES:
        assert e.obs_path(dtype, policy=True) == "fused"
        got = _run(e, snap, lambda: e.rollout_policy(K, 3, out=False, obs_dtype=dtype))
        _assert_same_but_obs(ref, got, dtype)


# ---- rounding classes: ideal_shape / ideal_vel reach the observation unchanged (static units), so exact patterns can be planted
def _f32(*patterns):
    return np.array(patterns, dtype=np.uint32).view(np.float32)


PLANTED = _f32(
    0x3F808000, 0x3F818000,             # bf16 ties: low half 0x8000 under an even / an odd upper half (1.00390625, 1.01171875)
    0x3F801000, 0x3F803000,             # fp16 ties: 1 + 2^-11 (to even: down), 1 + 3 * 2^-11 (to even: up)
    0xBF808000, 0xBF803000,             # ... and negative ones
    0x35800000, 0x33C00000,             # fp16 subnormal range: 2^-20; 1.5 * 2^-24, a tie between two subnormals
    0x33800000, 0xB8123456,             # 2^-24, the smallest subnormal; -3.48e-5
    0x32800000, 0x30800000,             # below 2^-25: 2^-26, 2^-30 round to +0
    0xB2800000, 0x33000000,             # -2^-26 rounds to -0; 2^-25 exactly, a tie that goes to the even 0
    0x477FE000, 0x477FF000,             # 65504, the largest fp16; 65520, which rounds to inf in fp16 and is finite in bf16
    0xC77FF000, 0x80000000)             # -65520; -0.0


def _classes(x):
    """Which rounding classes the fp32 tensor `x` holds: {name: bool}."""
    bits = x.contiguous().view(torch.int32)
    low16, odd16 = bits & 0xFFFF, (bits >> 16) & 1
    low13, odd13 = bits & 0x1FFF, (bits >> 13) & 1
    ax = x.abs()
    f16_normal = (ax >= 2.0 ** -14) & (ax <= 65504.0)
    return {
        "bf16 tie, even upper half": ((low16 == 0x8000) & (odd16 == 0)).any().item(),
        "bf16 tie, odd upper half": ((low16 == 0x8000) & (odd16 == 1)).any().item(),
        "fp16 tie, even": (f16_normal & (low13 == 0x1000) & (odd13 == 0)).any().item(),
        "fp16 tie, odd": (f16_normal & (low13 == 0x1000) & (odd13 == 1)).any().item(),
        "fp16 subnormal range": ((ax >= 2.0 ** -24) & (ax < 2.0 ** -14)).any().item(),
        "below 2^-25": ((ax > 0) & (ax < 2.0 ** -25)).any().item(),
        "65504": (x == 65504.0).any().item(),
        "65520": (x == 65520.0).any().item(),
        "-0.0": (bits == -2 ** 31).any().item(),
    }


def test_the_planted_values_land_in_their_classes():
    """On the CPU, with torch alone: the inputs of the next test are what its comments say."""
    x = torch.as_tensor(PLANTED.copy())
    assert all(_classes(x).values()), _classes(x)
    h, b = x.to(torch.float16), x.to(torch.bfloat16)
    assert h[0].item() == 1.0 + 2.0 ** -8 and h[2] == 1.0 and h[3].item() == 1.0 + 2.0 ** -9      # exact; ties to even
    assert b[0].item() == 1.0 and b[1].item() == 1.015625
    assert h[7].item() == 2.0 ** -23 and h[8].item() == 2.0 ** -24 and h[6].item() == 2.0 ** -20
    assert h[10] == 0 and h[11] == 0 and h[13] == 0 and _bits(h)[12].item() == -2 ** 15      # +0, +0, +0, -0
    assert h[14].item() == 65504.0 and torch.isinf(h[15]) and torch.isinf(h[16]) and torch.isfinite(b[15])
    assert _bits(h)[17].item() == -2 ** 15 and _bits(b)[17].item() == -2 ** 15


def test_rounding_classes():
    N, B = 9, 7
    e = _env(N, B, auto_reset=False)                       # no reset: the planted formation stays for all K steps
    shape = np.stack([np.roll(PLANTED, b) for b in range(B)]).reshape(B, N, 2)
    ivel = np.stack([np.roll(PLANTED, 3 * b + 1)[:2] for b in range(B)])
    e.scenario.set_formation(e.world, shape, ivel)
    assert np.array_equal(e.scenario.ideal_shape.cpu().numpy().view(np.uint32), shape.view(np.uint32))
    acts = _actions(e, seed=1)
    snap = e._snapshot()
    ref = _run(e, snap, lambda: e.rollout(acts, out=False))
    missing = [k for k, v in _classes(ref[0]).items() if not v]
    assert not missing, missing
    got = {}
    for dtype in DTYPES:
        assert e.obs_path(dtype) == "fused"
        got[dtype] = _run(e, snap, lambda: e.rollout(acts, out=False, obs_dtype=dtype))
        _assert_same_but_obs(ref, got[dtype], dtype)
    assert torch.isinf(got[torch.float16][0]).any() and torch.isfinite(got[torch.bfloat16][0]).all()      # 65520


# ---- the 'cast' route, and a caller's `out`
def _out(e, dtype, policy=False, pad=0):
    B, N = e.num_envs, e.num_agents
    D = e._out["obs"].shape[-1]
    f = dict(dtype=torch.float32, device=DEV)
    if pad:
        obs = torch.zeros((K, B, N * D + pad), dtype=dtype, device=DEV)[:, :, :N * D].unflatten(-1, (N, D))
        assert not obs.is_contiguous()
    else:
        obs = torch.zeros((K, B, N, D), dtype=dtype, device=DEV)
    out = dict(obs=obs, reward=torch.empty((K, B, N), **f), indiv=torch.empty((K, B, N), **f),
               done=torch.zeros((K, B, N), dtype=torch.uint8, device=DEV))
    if policy:
        out["act"] = torch.empty((K, B, N, 2), **f)
    return out


@pytest.mark.parametrize("name,N,B,want", [("formation_hd_env", 4, 5, "cast"), ("basic_formation_env", 3, 5, "cast"),
                                           ("formation_hd_env", 9, 7, "fused")])
def test_cast_route_and_callers_out(name, N, B, want):
    e = _env(N, B, name=name)
    acts = _actions(e)
    snap = e._snapshot()
    ref = _run(e, snap, lambda: e.rollout(acts, out=False))
    for dtype in DTYPES:
        assert e.obs_path(dtype) == want
        got = _run(e, snap, lambda: e.rollout(acts, out=False, obs_dtype=dtype))
        _assert_same_but_obs(ref, got, dtype)
        again = _run(e, snap, lambda: e.rollout(acts, obs_dtype=dtype))                 # out=None: fresh tensors as well
        _assert_same_but_obs(ref, again, dtype)
        assert again[0].data_ptr() != got[0].data_ptr()
        out = _out(e, dtype)
        mine = _run(e, snap, lambda: e.rollout(acts, out=out, obs_dtype=dtype))
        assert mine[0] is out["obs"]
        _assert_same_but_obs(ref, mine, dtype)
        assert torch.equal(out["indiv"], ref[3]["individual_reward"]) and torch.equal(out["done"].view(torch.bool), ref[2])
        e._restore(snap)
        with pytest.raises(ValueError):
            e.rollout(acts, out=_out(e, dtype, pad=16), obs_dtype=dtype)                # a padded env pitch
        with pytest.raises(ValueError):
            e.rollout(acts, out=_out(e, torch.float32), obs_dtype=dtype)                # out["obs"] of another dtype
    with pytest.raises(ValueError):
        e.rollout(acts, out=False, obs_dtype=torch.float64)
    one = _run(e, snap, lambda: e.rollout(acts[:1], out=False, obs_dtype=torch.float16))   # K = 1: always the cast
    e._restore(snap)
    assert torch.equal(_bits(one[0]), _bits(e.rollout(acts[:1], out=False)[0].to(torch.float16)))


def test_policy_cast_route_and_callers_out():
    for N, B, want in ((9, 7, "fused"), (4, 5, "cast")):
        e = _env(N, B)
        per = 3 if N == 9 else 2
        snap = e._snapshot()
        ref = _run(e, snap, lambda: e.rollout_policy(K, per, out=False))
        for dtype in DTYPES:
            assert e.obs_path(dtype, policy=True) == want
            out = _out(e, dtype, policy=True)
            mine = _run(e, snap, lambda: e.rollout_policy(K, per, out=out, obs_dtype=dtype))
            assert mine[0] is out["obs"]
            _assert_same_but_obs(ref, mine, dtype)
            e._restore(snap)
            with pytest.raises(ValueError):
                e.rollout_policy(K, per, out=_out(e, dtype, policy=True, pad=16), obs_dtype=dtype)


@pytest.mark.parametrize("N,B", SHAPES)
def test_two_launches_give_the_same_bits(N, B):
    e = _env(N, B)
    acts = _actions(e)
    snap = e._snapshot()
    for dtype in DTYPES:
        a = _run(e, snap, lambda: e.rollout(acts, out=False, obs_dtype=dtype))
        b = _run(e, snap, lambda: e.rollout(acts, out=False, obs_dtype=dtype))
        assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1])
