"""The planner on the GPU: the candidates' draws against the NumPy Philox reference, their composition, the sampled scoring
launch against `rollout_returns` on the materialised candidates (bit for bit: the test the feature rests on), MPPI's update against
a float64 two-pass reference, and `formation_gym.MPPIPlanner` end to end.  Every case is small."""
import numpy as np
import pytest
import torch

from formation_gym import MPPIPlanner, _native
from tests import counter_rng as cr
from tests import planner_testlib as pt
from tests import returns_testlib as rt
from tests.actor_testlib import params as _params

pytestmark = pytest.mark.gpu
DEV = rt.DEV
F32 = dict(dtype=torch.float32, device=DEV)


def _p(seed=cr.SEED, base=cr.BASE):
    p = _params()
    p.seed, p.env_index_base = seed, base
    return p


def _candidates(p, C, K, B, N, off, sigma=1.0, clip=0.0, mean=None):
    out = torch.empty((C, K, B, N, 2), **F32)
    _native.check(_native.load().fg_plan_candidates(p, B, N, K, C, off, sigma, clip, _native.ptr(mean), out.data_ptr(),
                                                    _native.current_stream(torch.device(DEV))))
    return out


def _mean(K, B, N, seed=1, scale=0.5):
    g = torch.Generator().manual_seed(977 * seed + K)
    return ((torch.rand((K, B, N, 2), generator=g) * 2 - 1) * scale).to(DEV)


# ---- 1. the draws ----
@pytest.mark.parametrize("off", cr.OFFSETS)
@pytest.mark.parametrize("C,K,B,N", [(7, 4, 5, 3), (3, 2, 4, 27), (2, 1, 2, 81), (4100, 1, 1, 3)])
def test_unit_draws_equal_the_numpy_reference(C, K, B, N, off):
    got = _candidates(_p(), C, K, B, N, off).double().cpu().numpy()
    want, r = pt.unit_draws(cr.SEED, cr.BASE, C, K, B, N, off)
    err = np.abs(got - want) / cr.gauss_bound(r)[..., None]
    print("C K B N = %s off %d: worst |eps - eps64| / gauss_bound(r) = %.3f" % ((C, K, B, N), off, err.max()))
    assert (err <= 1.0).all()
    other = _candidates(_p(), C, K, B, N, off + K).double().cpu().numpy()
    assert (np.abs(other - want) > cr.gauss_bound(r)[..., None]).mean() > 0.99      # another offset: other numbers


def test_planning_leaves_every_other_stream_alone():
    e = rt.env(3, 5, 4)
    before = [e.actor_noise().clone(), e.actor_uniform().clone(), e.actor_gumbel().clone()]   # Gaussian / OU, categorical, Gumbel
    MPPIPlanner(e, 4, 6, 0.7, 1.0).plan()
    for x, y in zip(before, [e.actor_noise(), e.actor_uniform(), e.actor_gumbel()]):
        assert torch.equal(x, y)


# ---- 2. the composition ----
def test_candidates_are_mean_plus_sigma_eps_clamped():
    C, K, B, N, off = 7, 4, 5, 3, 2 ** 32 - 2
    mean = _mean(K, B, N, scale=0.9)
    eps = _candidates(_p(), C, K, B, N, off).cpu()                       # the device's own unit draws (0 + 1 eps is exact)
    u = mean.cpu()[None] + eps * torch.tensor(0.7, dtype=torch.float32)      # one rounded product, one rounded sum
    got = _candidates(_p(), C, K, B, N, off, 0.7, 1.0, mean).cpu()
    assert torch.equal(got, torch.clamp(u, -1.0, 1.0))
    assert (u.abs() > 1.0).any() and (got.abs() == 1.0).any()            # the clamp bit
    assert torch.equal(_candidates(_p(), C, K, B, N, off, 0.7, 0.0, mean).cpu(), u)
    assert torch.equal(_candidates(_p(), C, K, B, N, off, 0.7, -1.0, mean).cpu(), u)
    assert torch.equal(_candidates(_p(), C, K, B, N, off, 0.0, 1.0, mean), mean[None].expand(C, K, B, N, 2))


# ---- 3. the sampled launch against the existing kernel ----
def _planner(e, K, C, gamma=0.97, off=2 ** 32 - 2, lam=1.0, sigma=0.7, mean_seed=1):
    pl = MPPIPlanner(e, K, C, sigma, lam, gamma=gamma, clip=1.0, noise_offset=off)
    pl.mean.copy_(_mean(K, e.num_envs, e.num_agents, mean_seed))
    return pl


def _sampled_equals_materialised(N, B, C, K, gamma):
    e = rt.env(N, B, K)
    pl = _planner(e, K, C, gamma)
    assert pl.path() == "fused"
    before = rt.env_facts(e)
    want, winfo = e.rollout_returns(pl.candidates(), gamma)
    got, ginfo = pl._score(pl.noise_offset, 0.7, gamma, 1.0)
    assert torch.equal(got, want) and torch.equal(ginfo["individual_return"], winfo["individual_return"])
    assert torch.equal(ginfo["steps"], winfo["steps"])
    assert torch.equal(ginfo["steps"].cpu(), rt.expected_steps(before[0]["step_count"].cpu(), K, int(e.world.world_length)))
    assert torch.isfinite(got).all()
    rt.assert_same_facts(before, rt.env_facts(e))
    return ginfo["steps"].tolist()


@pytest.mark.parametrize("gamma", [1.0, 0.97])
@pytest.mark.parametrize("N", rt.FUSED_N)
def test_sampled_launch_equals_returns_kernel(N, gamma):
    K = 6
    assert _sampled_equals_materialised(N, 5, 7, K, gamma) == [2, K, 1, K, K]     # episodes end inside the horizon; waves leave early


EDGES = {"C=1": (5, 1, 6), "K=1": (5, 7, 1), "K=2": (5, 7, 2), "K=3": (5, 7, 3), "K=5": (5, 7, 5), "K=7": (5, 7, 7),
         "B=1,C=130": (1, 130, 6)}


@pytest.mark.parametrize("N,shape", [(N, s) for N in (3, 27) for s in list(EDGES) + ["one more than a workgroup", "whole waves leave"]])
def test_sampled_launch_geometry_edges(N, shape):
    if shape == "one more than a workgroup":
        b, c, k = (5, 13, 6) if N == 3 else (5, 5, 6)
        assert (b * c) % (64 if N == 3 else 8) == 1
    elif shape == "whole waves leave":                  # env 2 (one counted step) owns whole waves beside waves that run all K
        b, c, k = (5, 32, 7) if N == 3 else (5, 4, 7)
    else:
        b, c, k = EDGES[shape]
    _sampled_equals_materialised(N, b, c, k, 0.97)


def test_a_bound_scoring_launch_follows_the_worlds_constants():
    """The fused route keeps its binding between `plan()` calls; a world constant written in between must reach it as it reaches
    `rollout_returns`, which builds its params per call."""
    N, B, C, K = 9, 5, 6, 4
    e = rt.env(N, B, K)
    pl = _planner(e, K, C)
    assert pl.path() == "fused"
    first = pl.plan()[1]["steps"].clone()
    pl.plan()                                           # both plan buffers hold a binding now
    assert first.tolist() == [2, K, 1, K, K]
    e.world.world_length = 39                           # env 4 (step counter 37) now ends inside the horizon
    e.world.damping = 0.5
    want, winfo = e.rollout_returns(pl.candidates(), 0.97)
    got, ginfo = pl._score(pl.noise_offset, 0.7, 0.97, 1.0)
    assert winfo["steps"].tolist() == [1, 1, 1, K, 2]
    assert torch.equal(ginfo["steps"], winfo["steps"]) and torch.equal(got, want)
    assert torch.equal(ginfo["individual_return"], winfo["individual_return"])
    action, info = pl.plan()
    assert torch.equal(info["returns"], want) and torch.isfinite(action).all()


# ---- 4. the update ----
def _update(p, ret, mean, off, sigma, clip, lam, shift):
    C, (K, B, N, _) = ret.shape[0], mean.shape
    buf = torch.zeros((2, K, B, N, 2), **F32)           # adjacent buffers: the first addresses that do not overlap
    buf[0].copy_(mean)
    act = torch.empty((B, N, 2), **F32)
    _native.check(_native.load().fg_plan_mppi_update(p, B, N, K, C, off, sigma, clip, lam, ret.data_ptr(), buf[0].data_ptr(),
                                                     buf[1].data_ptr(), act.data_ptr(), shift,
                                                     _native.current_stream(torch.device(DEV))))
    assert torch.equal(buf[0], mean)
    return buf[1].clone(), act


def _synthetic_returns(C, B, N):
    """[C,B,N] fp32 around -200: env 0 .. 2 spreads of 0, 1 and 30; env 3 an exact tie of the maximum; env 4 every other
    candidate 1e4 below the best."""
    g = torch.Generator().manual_seed(5 + C)
    r = torch.rand((C, B, N), generator=g)
    ret = torch.full((C, B, N), -200.0)
    for b, spread in ((1, 1.0), (2, 30.0)):
        ret[:, b] += (r[:, b] - 0.5) * spread
    ret[:, 3] += (r[:, 3] - 1.0)
    ret[0, 3] = -200.0
    ret[C - 1, 3] = -200.0                                 # candidates 0 and C - 1 tie at the top (one candidate: itself)
    ret[:, 4] = -10200.0 - r[:, 4]
    ret[C // 2, 4] = -200.0
    return ret


WORST = {}


def _check_update(ret, mean, off, sigma, clip, lam, tag):
    C, (K, B, N, _) = ret.shape[0], mean.shape
    p = _p()
    new0, act0 = _update(p, ret, mean, off, sigma, clip, lam, 0)
    new1, act1 = _update(p, ret, mean, off, sigma, clip, lam, 1)
    assert torch.equal(new1, pt.shifted(new0)) and torch.equal(act0, new0[0]) and torch.equal(act1, new0[0])
    eps, r = pt.unit_draws(cr.SEED, cr.BASE, C, K, B, N, off)
    u = pt.candidates64(mean.double().cpu().numpy(), np.float32(sigma), clip, eps)
    want, abar, umax = pt.mppi64(ret.double().cpu().numpy(), u, float(np.float32(lam)))
    bound = pt.mppi_bound(C, abar, umax, sigma, r.max(0))
    ratio = (np.abs(new0.double().cpu().numpy() - want) / bound[..., None]).max()
    WORST[tag] = max(WORST.get(tag, 0.0), ratio)
    print("%s C = %d lam = %g: worst |new - new64| / bound = %.3f" % (tag, C, lam, ratio))
    assert ratio <= 1.0, (tag, C, lam, ratio)


@pytest.mark.parametrize("C", [1, 2, 8, 130])
def test_update_against_float64_on_synthetic_returns(C):
    K, B, N, off = 3, 5, 3, 2 ** 32 - 2
    ret = _synthetic_returns(C, B, N).to(DEV)
    for lam in (0.05, 1.0, 1000.0):
        _check_update(ret, _mean(K, B, N, seed=C), off, 0.7, 1.0, lam, "synthetic")


@pytest.mark.parametrize("lam", [0.05, 1.0, 1000.0])
def test_update_against_float64_on_the_launchs_own_returns(lam):
    N, B, C, K, off = 3, 5, 8, 3, 5
    e = rt.env(N, B, K)
    e.scenario.env_base = cr.BASE
    pl = _planner(e, K, C, 0.97, off)
    ret = pl._score(off, 0.7, 0.97, 1.0)[0]
    assert int(e.scenario._seed) != 0
    p = e.scenario.params(e.world)
    eps, r = pt.unit_draws(int(p.seed), cr.BASE, C, K, B, N, off)
    u = pt.candidates64(pl.mean.double().cpu().numpy(), np.float32(0.7), 1.0, eps)
    want, abar, umax = pt.mppi64(ret.double().cpu().numpy(), u, float(np.float32(lam)))
    new, _ = _update(p, ret, pl.mean, off, 0.7, 1.0, lam, 0)
    ratio = (np.abs(new.double().cpu().numpy() - want) / pt.mppi_bound(C, abar, umax, 0.7, r.max(0))[..., None]).max()
    print("the launch's returns, lam = %g: worst |new - new64| / bound = %.3f" % (lam, ratio))
    assert ratio <= 1.0


# ---- 5. a small lambda picks the best candidate ----
def test_small_lambda_picks_the_best_candidate():
    d = pt.PICK
    N, B, C, K = d["N"], d["B"], d["C"], d["K"]
    e = rt.env(N, B, K, seed=d["seed"])
    st = pt.pick_state()
    e.scenario.set_formation(e.world, st["ideal_shape"], st["ideal_vel"])
    pl = MPPIPlanner(e, K, C, d["sigma"], d["lam"], gamma=d["gamma"], clip=d["clip"], noise_offset=d["noise_offset"])
    pl.mean.copy_(pt.pick_mean().to(DEV))
    cands = pl.candidates()
    best64, gap, _ = pt.pick_oracle()
    keep = torch.as_tensor(gap >= pt.GAP_FACTOR * d["lam"])             # [B]: the rows outside the excluded set
    assert keep.float().mean() >= 0.99
    action, info = pl.plan(shift=False)
    best = info["returns"].argmax(0).cpu()                                # [B,N]
    assert torch.equal(best[keep], torch.as_tensor(best64)[:, None].expand(B, N)[keep])
    idx = best.to(DEV)[None, None, :, :, None].expand(1, K, B, N, 2)
    want = torch.gather(cands, 0, idx)[0]                                 # [K,B,N,2]: the best candidate's action sequence
    assert torch.equal(pl.mean[:, keep.to(DEV)], want[:, keep.to(DEV)])
    assert torch.equal(action[keep.to(DEV)], want[0][keep.to(DEV)])


# ---- 6. the routes agree ----
def test_materialised_route_gives_the_fused_routes_bits():
    N, B, C, K = 9, 5, 6, 4
    fused, mat = _planner(rt.env(N, B, K), K, C), _planner(rt.env(N, B, K), K, C)
    mat.env._returns_replay_only = True
    assert (fused.path(), mat.path()) == ("fused", "materialised")
    for _ in range(2):
        (a0, i0), (a1, i1) = fused.plan(), mat.plan()
        assert torch.equal(a0, a1) and torch.equal(fused.mean, mat.mean)
        assert torch.equal(i0["returns"], i1["returns"]) and torch.equal(i0["individual_return"], i1["individual_return"])
        assert torch.equal(i0["steps"], i1["steps"]) and i0["noise_offset"] == i1["noise_offset"]
    assert fused.noise_offset == mat.noise_offset == 2 ** 32 - 2 + 2 * K


@pytest.mark.parametrize("name,N", [("basic_formation_env", 3), ("formation_hd_env", 5)])
def test_materialised_route_is_the_three_calls(name, N):
    B, C, K, gamma, lam = 5, 6, 4, 0.97, 0.5
    e = rt.env(N, B, K, name=name)
    pl, hand = _planner(e, K, C, gamma, lam=lam), _planner(e, K, C, gamma, lam=lam)
    assert pl.path() == "materialised"
    before = rt.env_facts(e)
    action, info = pl.plan()
    rt.assert_same_facts(before, rt.env_facts(e))
    cands = hand.candidates()
    ret, rinfo = e.rollout_returns(cands, gamma)
    new, act = _update(hand._params(), ret, hand.mean, hand.noise_offset, 0.7, 1.0, lam, 1)
    assert torch.equal(info["returns"], ret) and torch.equal(info["steps"], rinfo["steps"])
    assert torch.equal(action, act) and torch.equal(pl.mean, new)
    assert not torch.equal(new, hand.mean)


# ---- 7. a receding-horizon loop, twice ----
def _loop(off, rounds=6):
    N, B, C, K = 3, 8, 16, 5
    e = rt.env(N, B, K)
    e.auto_reset = True
    pl = MPPIPlanner(e, K, C, 0.5, 0.3, gamma=0.97, noise_offset=off)
    actions, resets = [], 0
    for _ in range(rounds):
        action, _ = pl.plan()
        done = e.step(action)[2]
        done = torch.as_tensor(done).reshape(B, -1)[:, 0].to(torch.bool)
        resets += int(done.sum())
        pl.reset(done)
        if done.any():
            assert not pl.mean[:, done.to(pl.mean.device)].any()
        actions.append(action.clone())
    assert pl.noise_offset == off + rounds * K
    return torch.stack(actions), e.world.get_state(), pl.mean.clone(), resets


def test_receding_horizon_loop_repeats_bit_for_bit():
    a0, s0, m0, resets = _loop(17)
    a1, s1, m1, _ = _loop(17)
    assert resets >= 1                                                    # an episode ended (auto-reset) inside the loop
    assert torch.equal(a0, a1) and torch.equal(m0, m1) and all(torch.equal(x, y) for x, y in zip(s0, s1))
    assert torch.isfinite(a0).all() and (a0.abs() <= 1.0).all() and a0.abs().max() > 0
    assert not torch.equal(_loop(18)[0], a0)                              # another noise_offset: other actions


# ---- 8. bad arguments ----
def test_bad_arguments_raise_and_launch_nothing():
    e = rt.env(3, 5, 4)
    pl = _planner(e, 4, 6)
    before, mean, off = rt.env_facts(e), pl.mean.clone(), pl.noise_offset
    for name, v in (("sigma", -1.0), ("sigma", float("nan")), ("lam", 0.0), ("gamma", 1.5)):
        old = getattr(pl, name)
        setattr(pl, name, v)
        with pytest.raises(ValueError):
            pl.plan()
        setattr(pl, name, old)
    out = dict(ret=torch.empty((6, 5, 3), **F32))
    with pytest.raises(_native.FormationHipError):
        e.scenario.bind_rollout_returns_sampled(e.world, pl.mean, pt.MAX_C + 1, out, 0.97)(0, 0.5, 1.0)
    with pytest.raises(_native.FormationHipError):
        e.scenario.bind_rollout_returns_sampled(e.world, pl.mean, 6, out, 0.97)(0, float("inf"), 1.0)
    with pytest.raises(_native.FormationHipError):                         # mean_out = mean_in
        _native.check(_native.load().fg_plan_mppi_update(pl._params(), 5, 3, 4, 6, 0, 0.5, 1.0, 1.0, out["ret"].data_ptr(),
                                                         pl.mean.data_ptr(), pl.mean.data_ptr(), None, 1, None))
    rt.assert_same_facts(before, rt.env_facts(e))
    assert torch.equal(pl.mean, mean) and pl.noise_offset == off
