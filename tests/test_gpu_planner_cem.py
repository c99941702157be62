"""The CEM planner on the GPU: the candidates with a sigma tensor against the NumPy Philox reference and against the scalar entry,
the sampled-std scoring launch against `fg_rollout_hd_returns` on the materialised candidates (bit for bit), the selection of
`fg_plan_cem_update` against the NumPy reference (exact, on every path and boundary of the kernel), its refit against float64
under a derived bound (tests/planner_cem_testlib.py: cem_bound), and `formation_gym.CEMPlanner` end to end.  Every case is small.

Worst |fp32 - fp64| / bound of the refit, as measured (profiles/planner_cem.md): see that file; the tests assert <= 1."""
import numpy as np
import pytest
import torch

from formation_gym import CEMPlanner, MPPIPlanner, _native
from tests import counter_rng as cr
from tests import planner_cem_testlib as ct
from tests import planner_testlib as pt
from tests import returns_testlib as rt
from tests.actor_testlib import params as _params

pytestmark = pytest.mark.gpu
DEV = rt.DEV
F32 = dict(dtype=torch.float32, device=DEV)
CAP, REG_C = _native.CEM_ELITE_CAP, _native.CEM_REG_C


def _stream():
    return _native.current_stream(torch.device(DEV))


def _p(seed=cr.SEED, base=cr.BASE):
    p = _params()
    p.seed, p.env_index_base = seed, base
    return p


def _candidates_std(p, C, off, clip, mean, std):
    K, B, N, _ = std.shape
    out = torch.empty((C, K, B, N, 2), **F32)
    _native.check(_native.load().fg_plan_candidates_std(p, B, N, K, C, off, clip, _native.ptr(mean), std.data_ptr(), out.data_ptr(),
                                                        _stream()))
    return out


def _candidates(p, C, K, B, N, off, sigma, clip, mean):
    out = torch.empty((C, K, B, N, 2), **F32)
    _native.check(_native.load().fg_plan_candidates(p, B, N, K, C, off, sigma, clip, _native.ptr(mean), out.data_ptr(), _stream()))
    return out


def _mean(K, B, N, seed=1, scale=0.5):
    g = torch.Generator().manual_seed(977 * seed + K)
    return ((torch.rand((K, B, N, 2), generator=g) * 2 - 1) * scale).to(DEV)


def _std(K, B, N, seed=1, scale=1.0):
    """Random in [0, scale] with about one exact zero in eight."""
    g = torch.Generator().manual_seed(313 * seed + K)
    s = torch.rand((K, B, N, 2), generator=g) * scale
    s[torch.rand((K, B, N, 2), generator=g) < 0.125] = 0.0
    return s.to(DEV)


# ---- 1. the candidates with a sigma tensor ----
@pytest.mark.parametrize("C,K,B,N", [(7, 4, 5, 3), (3, 2, 4, 27)])
def test_candidates_with_a_sigma_tensor_against_numpy(C, K, B, N):
    off, clip = 2 ** 32 - 2, 1.0
    mean, std = _mean(K, B, N, scale=0.9), _std(K, B, N)
    assert (std == 0).any() and (std > 0.5).any()
    eps, r = pt.unit_draws(cr.SEED, cr.BASE, C, K, B, N, off)
    m64, s64 = mean.double().cpu().numpy(), std.double().cpu().numpy()
    for mu, mu64 in ((mean, m64), (None, None)):                       # mean NULL: a zero mean
        got = _candidates_std(_p(), C, off, clip, mu, std).double().cpu().numpy()
        want = ct.candidates64_std(mu64, s64, clip, eps)
        amax = (0.0 if mu64 is None else np.abs(m64)[None]) + s64[None] * np.abs(eps)
        bound = s64[None] * cr.gauss_bound(r)[..., None] + ct.EPS * amax            # the draw, one product, one sum
        err = np.abs(got - want)
        print("C K B N = %s mean %s: worst |u - u64| / bound = %.3f" % ((C, K, B, N), mu is not None, (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all()
        assert (np.abs(got) <= clip).all() and (np.abs(got) == clip).any()
    zero = std.cpu().numpy() == 0
    got = _candidates_std(_p(), C, off, clip, mean, std).cpu().numpy()
    assert np.array_equal(got[:, zero], np.broadcast_to(mean.cpu().numpy()[zero], got[:, zero].shape))   # std 0: the mean itself


@pytest.mark.parametrize("C,K,B,N", [(7, 4, 5, 3), (3, 2, 4, 27)])
def test_a_constant_sigma_tensor_gives_the_scalar_entrys_bits(C, K, B, N):
    off, mean = 2 ** 32 - 2, _mean(K, B, N, scale=0.9)
    for sigma, clip in ((0.7, 1.0), (0.7, 0.0), (0.0, 1.0), (3.0, 1.0)):
        std = torch.full((K, B, N, 2), sigma, **F32)
        for mu in (mean, None):
            assert torch.equal(_candidates_std(_p(), C, off, clip, mu, std), _candidates(_p(), C, K, B, N, off, sigma, clip, mu))


# ---- 2. the sampled-std launch against the existing kernels ----
def _planner(e, K, C, E=3, gamma=0.97, off=2 ** 32 - 2, sigma=0.7, mean_seed=1, **kw):
    pl = CEMPlanner(e, K, C, min(E, C), sigma, gamma=gamma, clip=1.0, noise_offset=off, **kw)
    pl.mean.copy_(_mean(K, e.num_envs, e.num_agents, mean_seed))
    return pl


def _sampled_std_equals_materialised(N, B, C, K, gamma):
    e = rt.env(N, B, K)
    pl = _planner(e, K, C, gamma=gamma)
    pl.std.copy_(_std(K, B, N, scale=0.9))
    assert pl.path() == "fused"
    before = rt.env_facts(e)
    want, winfo = e.rollout_returns(pl.candidates(), gamma)
    got, ginfo = pl._score(pl.noise_offset, gamma, 1.0)
    assert torch.equal(got, want) and torch.equal(ginfo["individual_return"], winfo["individual_return"])
    assert torch.equal(ginfo["steps"], winfo["steps"]) and torch.isfinite(got).all()
    rt.assert_same_facts(before, rt.env_facts(e))
    # a constant sigma tensor: the scalar sampled launch's bits
    pl.std.fill_(0.7)
    got, ginfo = pl._score(pl.noise_offset, gamma, 1.0)
    got, indiv = got.clone(), ginfo["individual_return"].clone()
    mp = MPPIPlanner(e, K, C, 0.7, 1.0, gamma=gamma, clip=1.0, noise_offset=pl.noise_offset)
    mp.mean.copy_(pl.mean)
    ref, rinfo = mp._score(mp.noise_offset, 0.7, gamma, 1.0)
    assert torch.equal(got, ref) and torch.equal(indiv, rinfo["individual_return"])
    return ginfo["steps"].tolist()


@pytest.mark.parametrize("gamma", [1.0, 0.97])
@pytest.mark.parametrize("N", rt.FUSED_N)
def test_sampled_std_launch_equals_returns_kernel(N, gamma):
    K = 6
    assert _sampled_std_equals_materialised(N, 5, 7, K, gamma) == [2, K, 1, K, K]     # episodes end inside the horizon


@pytest.mark.parametrize("N,shape", [(N, s) for N in (3, 27) for s in ("K=1", "K=2", "K=3", "one more than a workgroup")])
def test_sampled_std_launch_geometry_edges(N, shape):
    if shape == "one more than a workgroup":
        b, c, k = (5, 13, 6) if N == 3 else (5, 5, 6)
        assert (b * c) % (64 if N == 3 else 8) == 1
    else:
        b, c, k = 5, 7, int(shape[2:])
    _sampled_std_equals_materialised(N, b, c, k, 0.97)


# ---- 3. the selection, exact ----
def _cem_update(p, ret, mean, std, E, off, clip, alpha, sigma_min, shift, act=True, elites=True):
    """One `fg_plan_cem_update` into adjacent buffers (the first addresses that do not overlap): (mean_out, std_out, act_out,
    elite_idx)."""
    C, (K, B, N, _) = ret.shape[0], mean.shape
    buf = torch.zeros((4, K, B, N, 2), **F32)
    buf[0].copy_(mean)
    buf[1].copy_(std)
    a = torch.empty((B, N, 2), **F32) if act else None
    idx = torch.full((E, B, N), -1, dtype=torch.int32, device=DEV) if elites else None
    _native.check(_native.load().fg_plan_cem_update(p, B, N, K, C, E, off, clip, alpha, sigma_min, ret.data_ptr(), buf[0].data_ptr(),
                                                    buf[1].data_ptr(), buf[2].data_ptr(), buf[3].data_ptr(), _native.ptr(a),
                                                    _native.ptr(idx), shift, _stream()))
    assert torch.equal(buf[0], mean) and torch.equal(buf[1], std)
    return buf[2].clone(), buf[3].clone(), a, idx


@pytest.mark.parametrize("C", [1, 2, 63, 64, 65, 130, 512, 513, REG_C, REG_C + 1, 4100])
def test_selection_is_exact(C):
    """Every row of the batch another pattern (two launches cover the seven); the E are those of `elite_counts`: the ends, the
    middle and the elite list's cap and one above it.  C: one, two and 64 keys per lane in registers, and re-read from memory."""
    K, B, N = 1, 2, 3
    mean, std = _mean(K, B, N), _std(K, B, N)
    for first in (0, 1):
        rows = ct.pattern_rows(C, first, B * N)
        ret = torch.as_tensor(rows.reshape(C, B, N)).to(DEV)
        for E in ct.elite_counts(C, CAP):
            want = ct.select(rows, E).reshape(E, B, N)
            idx = _cem_update(_p(), ret, mean, std, E, 5, 1.0, 1.0, 0.0, 0)[3].cpu().numpy()
            assert np.array_equal(idx, want), (C, E, first, [ct.PATTERNS[(first + j) % 7][0] for j in range(B * N)
                                                             if not np.array_equal(idx.reshape(E, -1)[:, j], want.reshape(E, -1)[:, j])])


def test_selection_places_every_nan_pattern_and_never_hangs():
    C, E, K, B, N = 130, 7, 1, 2, 3
    rng = np.random.default_rng(9)
    rows = rng.standard_normal((C, B * N)).astype(np.float32)
    bits = rows.view(np.uint32)
    bits[rng.integers(0, C, 20), rng.integers(0, B * N, 20)] = np.uint32(0x7FC00000)          # +NaN: above +inf
    bits[rng.integers(0, C, 20), rng.integers(0, B * N, 20)] = np.uint32(0xFFC00001)          # -NaN: below -inf
    rows[:, 5] = np.nan
    ret = torch.as_tensor(rows.reshape(C, B, N)).to(DEV)
    idx = _cem_update(_p(), ret, _mean(K, B, N), _std(K, B, N), E, 5, 1.0, 1.0, 0.0, 0)[3].cpu().numpy()
    assert np.array_equal(idx, ct.select(rows, E).reshape(E, B, N))


# ---- 4. the refit against float64 ----
WORST = {}


def _check_refit(ret, mean, std, E, off, clip, alpha, sigma_min, tag):
    C, (K, B, N, _) = ret.shape[0], mean.shape
    p = _p()
    m0, s0, a0, i0 = _cem_update(p, ret, mean, std, E, off, clip, alpha, sigma_min, 0)
    m1, s1, a1, i1 = _cem_update(p, ret, mean, std, E, off, clip, alpha, sigma_min, 1)
    assert torch.equal(m1, pt.shifted(m0)) and torch.equal(s1, pt.shifted(s0))
    assert torch.equal(a0, m0[0]) and torch.equal(a1, m0[0]) and torch.equal(i0, i1)
    again = _cem_update(p, ret, mean, std, E, off, clip, alpha, sigma_min, 0, act=False, elites=False)
    assert torch.equal(again[0], m0) and torch.equal(again[1], s0)                    # two launches: the same bits
    elite = ct.select(ret.cpu().numpy().reshape(C, -1), E).reshape(E, B, N)
    assert np.array_equal(i0.cpu().numpy(), elite)
    eps, r = pt.unit_draws(cr.SEED, cr.BASE, C, K, B, N, off)
    m64, s64 = mean.double().cpu().numpy(), std.double().cpu().numpy()
    u = ct.candidates64_std(m64, s64, clip, eps)
    al, smin = float(np.float32(alpha)), float(np.float32(sigma_min))
    want_m, want_s, m, s = ct.cem64(u, elite, m64, s64, al, smin)
    bm, bs = ct.cem_bound(u, eps, r, elite, m64, s64, al, m, s)
    rm = (np.abs(m0.double().cpu().numpy() - want_m) / bm).max()
    rs = (np.abs(s0.double().cpu().numpy() - want_s) / bs).max()
    WORST[tag] = np.maximum(WORST.get(tag, 0.0), (rm, rs))
    print("%s C = %d E = %d alpha = %g sigma_min = %g: worst |mean - mean64| / bound = %.3f, |std - std64| / bound = %.3f"
          % (tag, C, E, alpha, sigma_min, rm, rs))
    assert rm <= 1.0 and rs <= 1.0, (tag, C, E, alpha, sigma_min, rm, rs)
    return m0, s0, want_s


def _refit_returns(C, B, N):
    g = torch.Generator().manual_seed(5 + C)
    ret = -200.0 + 30.0 * torch.rand((C, B, N), generator=g)
    ret[:, 3] = torch.floor(ret[:, 3] / 8.0) * 8.0                                     # env 3: ties at the threshold
    return ret.to(DEV)


@pytest.mark.parametrize("C", [8, 130])
def test_refit_against_float64(C):
    K, B, N, off = 3, 5, 3, 2 ** 32 - 2
    ret, mean, std = _refit_returns(C, B, N), _mean(K, B, N, seed=C), _std(K, B, N, seed=C, scale=0.9)
    for E in (1, 3, C):
        for alpha in (1.0, 0.25):
            for sigma_min in (0.0, 5.0):                             # below and above every fitted value
                _, s0, want_s = _check_refit(ret, mean, std, E, off, 1.0, alpha, sigma_min, "refit")
                if sigma_min == 5.0:
                    assert (want_s == 5.0).all() and (s0 == 5.0).all()
                else:
                    assert (want_s < 5.0).all()


def test_refit_of_mostly_clamped_draws():
    C, E, K, B, N = 130, 40, 3, 5, 3
    std = torch.full((K, B, N, 2), 3.0, **F32)
    m0, s0, _ = _check_refit(_refit_returns(C, B, N), _mean(K, B, N), std, E, 7, 1.0, 1.0, 0.0, "clamped")
    cands = _candidates_std(_p(), C, 7, 1.0, _mean(K, B, N), std)
    assert (cands.abs() == 1.0).float().mean() > 0.6 and (s0 < 1.0).all()             # most draws clamped, the variance small


@pytest.mark.parametrize("C,E", [(8, 3), (130, 130), (130, 70)])
def test_refit_of_a_zero_std_gives_back_its_inputs(C, E):
    K, B, N = 3, 5, 3
    mean, std = _mean(K, B, N, seed=3, scale=0.9), torch.zeros((K, B, N, 2), **F32)
    for alpha in (1.0, 0.25):
        for sigma_min in (0.0, 0.125):
            m0, s0, _, _ = _cem_update(_p(), _refit_returns(C, B, N), mean, std, E, 7, 1.0, alpha, sigma_min, 0)
            assert torch.equal(m0, mean) and torch.equal(s0, torch.full_like(s0, sigma_min))      # max(sigma_min, (1 - alpha) 0)


def test_all_elites_and_alpha_one_is_the_plain_mean_like_mppi_at_a_large_lambda():
    """For the record, printed and not asserted beyond the bound: E = C, alpha = 1 is MPPI's update as lam -> inf."""
    C, K, B, N, off = 8, 3, 5, 3, 11
    ret, mean = _refit_returns(C, B, N), _mean(K, B, N)
    std = torch.full((K, B, N, 2), 0.7, **F32)
    m0 = _cem_update(_p(), ret, mean, std, C, off, 1.0, 1.0, 0.0, 0)[0]
    out = torch.empty_like(mean)
    _native.check(_native.load().fg_plan_mppi_update(_p(), B, N, K, C, off, 0.7, 1.0, 1e6, ret.data_ptr(), mean.data_ptr(),
                                                     out.data_ptr(), None, 0, _stream()))
    plain = _candidates(_p(), C, K, B, N, off, 0.7, 1.0, mean).double().mean(0)
    print("E = C, alpha = 1: max |cem - plain mean| = %.3g;  max |mppi(lam = 1e6) - plain mean| = %.3g"
          % ((m0.double() - plain).abs().max(), (out.double() - plain).abs().max()))
    assert (m0.double() - plain).abs().max() < 1e-5


# ---- 5. CEMPlanner end to end ----
def _hand_chain(e, pl, off, iterations, shift, gamma=0.97, E=3, alpha=1.0, sigma_min=0.0, sigma=0.7):
    """`iterations` rounds of the three C calls from pl's mean: (action, mean, std, returns, elites)."""
    lib, p = _native.load(), pl._params()
    B, N, K, C = pl._dims()
    mean, std = pl.mean.clone(), torch.full_like(pl.mean, sigma)
    for j in range(iterations):
        o = off + j * K
        cands = _candidates_std(p, C, o, 1.0, mean, std)
        ret, info = e.rollout_returns(cands, gamma)
        ret = ret.contiguous()
        mean, std, act, idx = _cem_update(p, ret, mean, std, E, o, 1.0, alpha, sigma_min, int(shift and j == iterations - 1))
    return act, mean, std, ret, idx, info


@pytest.mark.parametrize("iterations", [1, 3])
def test_plan_is_the_hand_chain_of_the_three_calls(iterations):
    N, B, K, C, off = 3, 5, 3, 8, 2 ** 32 - 2
    e = rt.env(N, B, K)
    pl = _planner(e, K, C, iterations=iterations)
    assert pl.path() == "fused"
    before = rt.env_facts(e)
    act, mean, std, ret, idx, rinfo = _hand_chain(e, pl, off, iterations, True)
    action, info = pl.plan()
    rt.assert_same_facts(before, rt.env_facts(e))                      # state, step counters and RNG offset untouched
    assert torch.equal(action, act) and torch.equal(pl.mean, mean) and torch.equal(pl.std, std) and info["std"] is pl.std
    assert torch.equal(info["returns"], ret) and torch.equal(info["elites"], idx) and torch.equal(info["steps"], rinfo["steps"])
    assert info["noise_offset"] == off and pl.noise_offset == off + iterations * K
    assert np.array_equal(info["elites"].cpu().numpy(),
                          ct.select(info["returns"].cpu().numpy().reshape(C, -1), 3).reshape(3, B, N))
    assert not torch.equal(mean, _mean(K, B, N)) and (std != 0.7).any()


def test_materialised_route_gives_the_fused_routes_bits():
    N, B, C, K = 9, 5, 6, 4
    fused, mat = _planner(rt.env(N, B, K), K, C, alpha=0.5, sigma_min=0.05), _planner(rt.env(N, B, K), K, C, alpha=0.5, sigma_min=0.05)
    mat.env._returns_replay_only = True
    assert (fused.path(), mat.path()) == ("fused", "materialised")
    for _ in range(2):
        (a0, i0), (a1, i1) = fused.plan(), mat.plan()
        assert torch.equal(a0, a1) and torch.equal(fused.mean, mat.mean) and torch.equal(fused.std, mat.std)
        for k in ("returns", "individual_return", "steps", "std", "elites"):
            assert torch.equal(i0[k], i1[k]), k
        assert i0["noise_offset"] == i1["noise_offset"]
    assert fused.noise_offset == mat.noise_offset == 2 ** 32 - 2 + 2 * 3 * K


@pytest.mark.parametrize("name,N", [("basic_formation_env", 3), ("formation_hd_env", 5)])
def test_materialised_route_runs_where_nothing_is_fused(name, N):
    B, C, K = 5, 8, 3
    e = rt.env(N, B, K, name=name)
    pl = _planner(e, K, C, iterations=2)
    assert pl.path() == "materialised"
    before = rt.env_facts(e)
    act, mean, std, ret, idx, _ = _hand_chain(e, pl, pl.noise_offset, 2, True)
    action, info = pl.plan()
    rt.assert_same_facts(before, rt.env_facts(e))
    assert torch.equal(action, act) and torch.equal(pl.mean, mean) and torch.equal(pl.std, std)
    assert torch.equal(info["returns"], ret) and torch.equal(info["elites"], idx)
    assert torch.isfinite(action).all() and (action.abs() <= 1.0).all()


def _loop(off, rounds=4):
    N, B, C, K = 3, 5, 8, 3
    e = rt.env(N, B, K)
    pl = CEMPlanner(e, K, C, 3, 0.5, iterations=2, alpha=0.8, sigma_min=0.01, gamma=0.97, noise_offset=off)
    actions = []
    for _ in range(rounds):
        action, _ = pl.plan()
        e.step(action)
        actions.append(action.clone())
    assert pl.noise_offset == off + rounds * 2 * K
    return torch.stack(actions), e.world.get_state(), pl.mean.clone(), pl.std.clone()


def test_receding_horizon_loop_repeats_bit_for_bit():
    a0, s0, m0, d0 = _loop(17)
    a1, s1, m1, d1 = _loop(17)
    assert torch.equal(a0, a1) and torch.equal(m0, m1) and torch.equal(d0, d1) and all(torch.equal(x, y) for x, y in zip(s0, s1))
    assert torch.isfinite(a0).all() and (a0.abs() <= 1.0).all() and a0.abs().max() > 0
    assert not torch.equal(_loop(18)[0], a0)                              # another noise_offset: other actions


def test_bad_arguments_raise_and_launch_nothing():
    e = rt.env(3, 5, 3)
    pl = _planner(e, 3, 8)
    before, mean, std, off = rt.env_facts(e), pl.mean.clone(), pl.std.clone(), pl.noise_offset
    for name, v in (("sigma", -1.0), ("elites", 9), ("elites", 0), ("alpha", 0.0), ("sigma_min", float("nan")), ("iterations", 0),
                    ("gamma", 1.5)):
        old = getattr(pl, name)
        setattr(pl, name, v)
        with pytest.raises(ValueError):
            pl.plan()
        setattr(pl, name, old)
    out = dict(ret=torch.empty((8, 5, 3), **F32))
    with pytest.raises(_native.FormationHipError):
        e.scenario.bind_rollout_returns_sampled_std(e.world, pl.mean, pl.std, pt.MAX_C + 1, out)(0, 0.97, 1.0)
    with pytest.raises(_native.FormationHipError):
        e.scenario.bind_rollout_returns_sampled_std(e.world, pl.mean, pl.std, 8, out)(0, 1.5, 1.0)
    with pytest.raises(_native.FormationHipError):                         # mean_out = mean_in
        _native.check(_native.load().fg_plan_cem_update(pl._params(), 5, 3, 3, 8, 3, 0, 1.0, 1.0, 0.0, out["ret"].data_ptr(),
                                                        pl.mean.data_ptr(), pl.std.data_ptr(), pl.mean.data_ptr(),
                                                        pl._std_spare.data_ptr(), None, None, 1, None))
    rt.assert_same_facts(before, rt.env_facts(e))
    assert torch.equal(pl.mean, mean) and torch.equal(pl.std, std) and pl.noise_offset == off
