"""GPU tests of the OU-noise actor rollout: `env.rollout_actor(K, OUNoiseActor(inner, ...), noise_state=x)` - the MADDPG trainers'
exploration, x <- x + theta (mu - x) + sigma eps, a = clamp(inner(o) + scale x, -clip, clip) - fused on the four families without
LayerNorms (`fg_rollout_hd_actor_ou`: ou_actor_kernel, bn_ou_actor_kernel; `fg_rollout_hd_actor_ou_per_agent`: pa_ou_actor_kernel,
pa_bn_ou_actor_kernel) and host-paced elsewhere.

References and bounds (tests/actor_ou_testlib.py).  The state's reference is a free-running fp64 recursion from the given x0 on
the replayed draws `noise_at(env, k)`, reset to mu by the launch's own done flags; the final state must meet
    |x32 - x64| <= 4 * 2^-24 * M / theta,    M = max(1, |mu|, max |x64|, sigma max |eps|) over the launch
(three roundings per step under a contraction of 1 - theta).  The actions' reference is clamp(inner64(o_k) + scale x64_k, +-clip)
on the observation step k acted on; the tolerance is the inner family's existing actor bound - 1e-5 max(1, |a64|), times
max(1, s) behind an input BatchNorm - plus `scale` times the state bound, the clamp being 1-Lipschitz.  Each test prints its
largest err / bound before it asserts <= 1.

The cases' parameters theta = 0.15, mu = 0.05, sigma = 0.3, scale = 0.5, clip = 1 are chosen so that every case has actions at
+clip, at -clip and strictly inside (asserted), and a non-zero mu, so that a reset to mu differs from a reset to zero.  Every
env's launch has an episode end inside it (actor_testlib.env) and a third of the envs one at its last step.

Host-paced twin.  Both paths evaluate the same fp32 function on the same observation only at step 0, so with a real inner actor
the twin is compared there, within twice the bound; with a zeroed inner actor the actions are the noise itself and both
trajectories - actions and noise_state - are the same bits over all K steps, because the host-paced loop steps the state with the
kernels' own device function (`fg_actor_ou_step`).
"""
import functools

import pytest
import torch

from formation_gym import OUNoiseActor
from tests import actor_ou_testlib as ot
from tests.actor_testlib import (B, DEV, K, Wrap as _Wrap, clone as _clone, current_obs as _current_obs, env as _env,
                                 hand_loop as _hand_loop, noise_at as _noise_at, obs_before as _obs_before, scaled_mlp,
                                 state as _state)

pytestmark = pytest.mark.gpu

THETA, MU, SIGMA, SCALE, CLIP = 0.15, 0.05, 0.3, 0.5, 1.0
# (family, N, H, tanh): shared N = 3 (E = 64), 9 (5 tiles: a wave owns two), 27 (E = 8, 7 tiles, ragged last tile); per agent
# N = 9 (agent-major rows, EP = 16), 27 (half-full tiles); shared BatchNorm N = 9; per-agent BatchNorm N = 4
CASES = [("shared", 3, 64, True), ("shared", 9, 64, False), ("shared", 27, 32, True), ("per_agent", 9, 64, False),
         ("per_agent", 27, 64, True), ("bn", 9, 32, False), ("pa_bn", 4, 64, True)]
IDS = ["%s-N%d-H%d-tanh%d" % c for c in CASES]


def _ou(inner, **kw):
    d = dict(theta=THETA, sigma=SIGMA, scale=SCALE, mu=MU, clip=CLIP)
    d.update(kw)
    return OUNoiseActor(inner, **d)


def _ou_env(N, last_step_done=True):
    """actor_testlib.env, with every third env (from 1) ending an episode at the last step of a K-step launch."""
    e = _env(N)
    if last_step_done:
        e.world.step_count[1::3] = int(e.world.world_length) - K
    return e


def _x0(N, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (0.3 * torch.randn(B, N, 2, generator=g)).to(DEV)


def _check_against_fp64(ou, x0, eps, obs0, obs, done, acts, x_end, tag):
    """The state and action checks of the module docstring for one launch's results; returns the two err / bound figures."""
    clip = float("inf") if ou.clip is None else ou.clip
    used64, end64 = ot.ou_reference(ou.theta, ou.mu, ou.sigma, x0, eps, done)
    sb = ot.state_bound(ou.theta, ou.mu, ou.sigma, used64, eps)
    s_ratio = float((x_end.double() - end64).abs().max()) / sb
    print("OU %s state max err/bound = %.4f (bound %.3g)" % (tag, s_ratio, sb))
    a_ratio = 0.0
    for k, o in enumerate(_obs_before(obs0, obs, len(acts))):
        mean64, bound = ot.mean_and_bound(ou.actor, o)
        want = (mean64 + ou.scale * used64[k]).clamp(-clip, clip)
        a_ratio = max(a_ratio, float(((acts[k].double() - want).abs() / (bound + abs(ou.scale) * sb)).max()))
        sure = (mean64 + ou.scale * used64[k]).abs() > clip + bound + abs(ou.scale) * sb      # clamped on either side of the error
        assert torch.equal(acts[k][sure].abs(), torch.full_like(acts[k][sure], clip)), "step %d: a clamped value is not +-clip" % k
    print("OU %s action max err/bound = %.4f" % (tag, a_ratio))
    assert s_ratio <= 1.0 and a_ratio <= 1.0, "%s: state %.3g, action %.3g of the bound" % (tag, s_ratio, a_ratio)
    return s_ratio, a_ratio


@functools.lru_cache(maxsize=None)
def _launch(case):
    """One fused K-step launch of `case` from a snapshot, computed once and shared by the tests below (nothing in it is
    modified afterwards): the env, actor, snapshot, x0, the replayed draws, obs0, the results and the final simulator state."""
    kind, N, H, tanh = case
    env = _ou_env(N)
    ou = _ou(ot.inner_actor(kind, N, H, tanh, seed=N))
    assert env.actor_path(ou) == "fused"
    snap = env._snapshot()
    x0 = _x0(N)
    eps = torch.stack([_noise_at(env, k) for k in range(K)])
    obs0 = _current_obs(env)
    x = x0.clone()
    res = env.rollout_actor(K, ou, noise_state=x)
    in_place = res[3]["noise_state"] is x
    obs, rew, done, info = _clone(res)
    return dict(env=env, ou=ou, snap=snap, x0=x0, eps=eps, obs0=obs0, obs=obs, rew=rew, done=done, info=info,
                x_end=x.clone(), state=_state(env), in_place=in_place)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_path_replay_and_determinism(case):
    r = _launch(case)
    env, info = r["env"], r["info"]
    assert r["in_place"] and "log_prob" not in info and info["actions"].shape == (K, B, case[1], 2)
    assert bool(r["done"].any()) and bool(r["done"][K - 1].any()) and not bool(r["done"][K - 1].all())
    env._restore(r["snap"])
    r_obs, r_rew, r_done, r_info = env.rollout(info["actions"].clone())
    assert torch.equal(r["obs"], r_obs) and torch.equal(r["rew"], r_rew) and torch.equal(r["done"], r_done)
    assert torch.equal(info["individual_reward"], r_info["individual_reward"])
    for a, b in zip(r["state"], _state(env)):
        assert torch.equal(a, b)
    env._restore(r["snap"])
    x = r["x0"].clone()
    obs2, rew2, _, info2 = env.rollout_actor(K, r["ou"], noise_state=x)
    assert torch.equal(info["actions"], info2["actions"]) and torch.equal(r["obs"], obs2) and torch.equal(r["rew"], rew2)
    assert torch.equal(x, r["x_end"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_state_and_actions_against_fp64(case):
    r = _launch(case)
    acts = r["info"]["actions"]
    _check_against_fp64(r["ou"], r["x0"], r["eps"], r["obs0"], r["obs"], r["done"], acts, r["x_end"], IDS[CASES.index(case)])
    # the clamp is exercised on both sides and left alone in between, and nothing leaves [-clip, clip]
    assert bool((acts == CLIP).any()) and bool((acts == -CLIP).any()) and bool((acts.abs() < CLIP).any())
    assert float(acts.abs().max()) == CLIP


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_launch_equals_k_one_step_launches(case):
    r = _launch(case)
    env = r["env"]
    env._restore(r["snap"])
    x = r["x0"].clone()
    acts, obss = [], []
    for _ in range(K):
        obs, _, _, info = env.rollout_actor(1, r["ou"], noise_state=x)
        acts.append(info["actions"][0].clone())
        obss.append(obs[0].clone())
    assert torch.equal(torch.stack(acts), r["info"]["actions"]) and torch.equal(torch.stack(obss), r["obs"])
    assert torch.equal(x, r["x_end"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_rows_of_finished_episodes_hold_mu(case):
    r = _launch(case)
    last = r["done"][K - 1]                                                # [B, N] (or [B, N, 1])
    last = last.reshape(B, case[1])
    mu32 = torch.tensor(MU, dtype=torch.float32, device=DEV)
    assert bool((r["x_end"][last] == mu32).all()), "a finished episode's rows are not exactly mu"
    assert bool((r["x_end"][~last] != mu32).any(-1).all()), "a running episode's row was reset"


def test_state_is_reset_without_auto_reset_too():
    N = 9
    env = _ou_env(N)
    env.auto_reset = False
    ou = _ou(ot.inner_actor("shared", N, 64, False, seed=N))
    assert env.actor_path(ou) == "fused"
    x = _x0(N)
    _, _, done, _ = env.rollout_actor(K, ou, noise_state=x)
    last = done[K - 1].reshape(B, N)
    assert bool(last.any()) and not bool(last.all())
    assert bool((x[last] == torch.tensor(MU, dtype=torch.float32, device=DEV)).all())


@pytest.mark.parametrize("kind,N,H", [("shared", 9, 64), ("per_agent", 9, 64), ("bn", 27, 32), ("pa_bn", 4, 64)])
def test_host_paced_twin(kind, N, H):
    env = _ou_env(N)
    for zero in (True, False):
        inner = ot.inner_actor(kind, N, H, False, seed=3, zero=zero)
        fused, host = _ou(inner), _ou(_Wrap(inner))
        assert env.actor_path(fused) == "fused" and env.actor_path(host) == "host"
        snap = env._snapshot()
        obs0 = _current_obs(env)
        xf, xh = _x0(N), _x0(N)
        f = _clone(env.rollout_actor(K, fused, noise_state=xf))
        env._restore(snap)
        h = env.rollout_actor(K, host, noise_state=xh)
        assert h[3]["noise_state"] is xh and "log_prob" not in h[3]
        if zero:                                                           # the actions are the noise itself: the same bits
            assert torch.equal(h[3]["actions"], f[3]["actions"]) and torch.equal(xh, xf)
            assert torch.equal(h[0], f[0]) and torch.equal(h[1], f[1]) and torch.equal(h[2], f[2])
            assert bool((f[3]["actions"].abs() > 0).any())
        else:
            _, bound = ot.mean_and_bound(inner, obs0)
            diff = (h[3]["actions"][0].double() - f[3]["actions"][0].double()).abs()
            print("OUTWIN %s N=%d max diff/(2 bound) at step 0 = %.4f" % (kind, N, float((diff / (2 * bound)).max())))
            assert bool((diff <= 2 * bound).all())
        env._restore(snap)


def test_scalars_are_read_in_place_by_the_bound_launcher():
    N = 9
    env = _ou_env(N)
    ou = _ou(ot.inner_actor("bn", N, 64, False, seed=6))
    f = dict(dtype=torch.float32, device=DEV)
    out = dict(obs=torch.empty((K, B, N, 6 * N), **f), reward=torch.empty((K, B, N), **f), indiv=torch.empty((K, B, N), **f),
               done=torch.zeros((K, B, N), dtype=torch.uint8, device=DEV), act=torch.empty((K, B, N, 2), **f))
    x = _x0(N)
    snap = env._snapshot()

    def run(tag):
        env._restore(snap)
        x.copy_(_x0(N))
        x0, obs0 = x.clone(), _current_obs(env)
        eps = torch.stack([_noise_at(env, k) for k in range(K)])
        obs, _, done, info = env.rollout_actor(K, ou, out=out, noise_state=x)
        assert info["noise_state"] is x
        _check_against_fp64(ou, x0, eps, obs0, obs, done, info["actions"], x, "in-place " + tag)
        return info["actions"].clone(), x.clone()
    first = run("first")
    bound = dict(env._roll_launchers)
    assert len(bound) == 1
    ou.scale, ou.sigma = 0.125, 0.45                                       # an annealed scale, another sigma
    second = run("annealed")
    assert dict(env._roll_launchers) == bound, "the same buffers and module must reuse the bound launcher"
    assert not torch.equal(first[0], second[0]) and not torch.equal(first[1], second[1])


def test_no_clip_and_the_memoryless_special_case():
    N = 9
    env = _ou_env(N)
    unclipped = _ou(ot.inner_actor("shared", N, 64, False, seed=N), clip=None)
    assert env.actor_path(unclipped) == "fused"
    snap = env._snapshot()
    acts = env.rollout_actor(K, unclipped, noise_state=_x0(N))[3]["actions"]
    assert float(acts.abs().max()) > 1.0 and bool(torch.isfinite(acts).all())
    # theta = 1, mu = 0: x = sigma eps at every step (maddpg-v1's noise); a zeroed inner actor, scale 1 and no clamp show x
    env._restore(snap)
    iid = OUNoiseActor(ot.inner_actor("shared", N, 64, False, zero=True), theta=1.0, sigma=SIGMA, scale=1.0, mu=0.0, clip=None)
    want = torch.stack([SIGMA * _noise_at(env, k) for k in range(K)])
    x = _x0(N)
    obs, _, done, info = env.rollout_actor(K, iid, noise_state=x)
    assert env.actor_path(iid) == "fused" and torch.equal(info["actions"], want)
    last = done[K - 1].reshape(B, N)
    assert torch.equal(x[~last], want[K - 1][~last]) and bool((x[last] == 0).all())


def test_errors_and_the_landmark_fallback():
    N = 9
    env = _ou_env(N)
    plain = ot.inner_actor("shared", N, 64, True)
    ou = _ou(plain)
    with pytest.raises(ValueError):
        env.rollout_actor(K, plain, noise_state=_x0(N))
    bad = [torch.zeros(B, N, 3, device=DEV), torch.zeros(B, N, 2, device=DEV, dtype=torch.float64), torch.zeros(B, N, 2),
           torch.zeros(B, 2, N, device=DEV).transpose(1, 2), torch.zeros(B + 1, N, 2, device=DEV)]
    for x in bad:
        with pytest.raises(ValueError):
            env.rollout_actor(K, ou, noise_state=x)
    fresh = env.rollout_actor(2, ou)[3]["noise_state"]                      # None: a fresh initial_state per call
    assert fresh.shape == (B, N, 2) and fresh.dtype == torch.float32
    # a landmark scenario has no OU kernel: host-paced, with the hand loop's results.  theta = 1, mu = 0 makes the hand
    # loop's torch arithmetic exact (x = sigma eps), so the comparison is bit for bit over all steps
    lm = _env(3, name="basic_formation_env")
    D = lm._out["obs"].shape[-1]
    inner = scaled_mlp(D, 64, True, seed=2)
    assert lm.actor_path(inner) == "fused"
    ou_lm = OUNoiseActor(inner, theta=1.0, sigma=0.4, scale=0.5, mu=0.0, clip=1.0)
    assert lm.actor_path(ou_lm) == "host"
    snap = lm._snapshot()

    def by_hand(o):
        return (inner(o) + 0.5 * (0.4 * _noise_at(lm, 0))).clamp(-1.0, 1.0)
    acts, obss, rews = _hand_loop(lm, by_hand, K)
    lm._restore(snap)
    obs, rew, _, info = lm.rollout_actor(K, ou_lm)
    assert torch.equal(info["actions"], acts) and torch.equal(obs, obss) and torch.equal(rew, rews)
    assert bool((acts.abs() == 1.0).any()) and bool((acts.abs() < 1.0).any())
