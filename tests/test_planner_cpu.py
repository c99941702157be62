"""CPU checks of the planner entries (`fg_rollout_hd_returns_sampled` and its dry run, `fg_plan_candidates`,
`fg_plan_mppi_update`) and of `formation_gym.MPPIPlanner`: the symbols, the dry run against `fg_describe_returns_launch`, every
argument check that precedes a launch, the planner's host logic on a stand-in env, the stream code against every other stream's,
and the condition the inputs of the GPU test "a small lambda picks the best candidate" must meet.  No device is touched."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from formation_gym import MPPIPlanner, _native
from tests import counter_rng as cr
from tests import planner_testlib as pt
from tests import returns_testlib as rt
from tests.actor_testlib import ROOT, params as _params

P = 4096                                                   # a stand-in address: only NULL-ness, alignment and ranges are looked at
FAR = 1 << 30                                              # ... and one far from it
OK, BAD, UNSUPPORTED, ALIGN = _native.FG_OK, _native.FG_ERR_BAD_ARG, _native.FG_ERR_UNSUPPORTED_N, _native.FG_ERR_ALIGNMENT
NEW = ("fg_rollout_hd_returns_sampled", "fg_describe_returns_sampled_launch", "fg_plan_candidates", "fg_plan_mppi_update")


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def _p(**kw):
    p = _params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_symbols_are_exported_bound_and_documented(lib):
    header = open(os.path.join(ROOT, "include", "formation_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in _native.SIGNATURES and ("int %s(" % name) in header and name in doc, name
    assert lib.fg_abi_version() == _native.ABI_VERSION == 8           # entries added, no struct changed
    assert (_native.PLAN_MAX_N, _native.PLAN_MAX_C) == (pt.MAX_N, pt.MAX_C)


# ---- the dry run ----
def _describe(lib, fn, p, B, N, K, C):
    buf = ctypes.create_string_buffer(256)
    rc = getattr(lib, fn)(p, B, N, K, C, buf, 256)
    return rc, buf.value.decode()


@pytest.mark.parametrize("N", rt.FUSED_N)
def test_dry_run_is_the_returns_kernels_with_the_name_changed(lib, N):
    for B, C in ((5, 7), (1, 1), (1, 4096), (4096, 8), (16384, 16), (1, 130), (1, pt.MAX_C)):
        rc, text = _describe(lib, "fg_describe_returns_launch", _p(), B, N, 20, C)
        rc_s, text_s = _describe(lib, "fg_describe_returns_sampled_launch", _p(), B, N, 20, C)
        assert rc == rc_s == OK and text.startswith("returns_kernel<")
        assert text_s == text.replace("returns_kernel<", "returns_sampled_kernel<", 1)


def test_dry_run_status_codes(lib):
    for kw, B, N, C in ((dict(), 4, 5, 3), (dict(), 4, 81, 3), (dict(u_noise=0.1), 4, 9, 3), (dict(num_walls=1), 4, 9, 3),
                        (dict(agent_props=P), 4, 9, 3), (dict(), 70000, 9, 70000), (dict(), -1, 9, 3), (dict(), 4, 9, 0)):
        want = _describe(lib, "fg_describe_returns_launch", _p(**kw), B, N, 5, C)
        got = _describe(lib, "fg_describe_returns_sampled_launch", _p(**kw), B, N, 5, C)
        assert want[0] != OK and got == (want[0], ""), (kw, B, N, C)
    assert _describe(lib, "fg_describe_returns_launch", _p(), 1, 9, 5, pt.MAX_C + 1)[0] == OK
    assert _describe(lib, "fg_describe_returns_sampled_launch", _p(), 1, 9, 5, pt.MAX_C + 1) == (BAD, "")
    assert "C <= 2^17" in lib.fg_last_error().decode()
    assert _describe(lib, "fg_describe_returns_sampled_launch", None, 1, 9, 5, 3)[0] == BAD
    assert lib.fg_describe_returns_sampled_launch(_p(), 1, 9, 5, 3, None, 0) == BAD
    assert _describe(lib, "fg_describe_returns_sampled_launch", _p(), 0, 9, 5, 3) == (OK, "")


# ---- the argument checks that precede a launch ----
def _sampled(lib, params="default", B=4, N=9, K=5, C=3, gamma=0.9, off=7, sigma=0.5, clip=1.0, **ptrs):
    names = ("pos_x", "pos_y", "vel_x", "vel_y", "ideal_shape", "ideal_vel", "step", "mean", "ret", "indiv_ret", "steps")
    assert set(ptrs) <= set(names)
    p = _p() if params == "default" else params
    return lib.fg_rollout_hd_returns_sampled(p, B, N, K, C, gamma, off, sigma, clip, *[ptrs.get(k, P) for k in names], None)


def _candidates(lib, params="default", B=4, N=9, K=5, C=3, off=7, sigma=0.5, clip=1.0, mean=P, act=FAR):
    return lib.fg_plan_candidates(_p() if params == "default" else params, B, N, K, C, off, sigma, clip, mean, act, None)


def _update(lib, params="default", B=4, N=9, K=5, C=3, off=7, sigma=0.5, clip=1.0, lam=1.0, ret=P, mean_in=FAR, mean_out=2 * FAR,
            act=3 * FAR, shift=1):
    return lib.fg_plan_mppi_update(_p() if params == "default" else params, B, N, K, C, off, sigma, clip, lam, ret, mean_in,
                                   mean_out, act, shift, None)


ENTRIES = (_sampled, _candidates, _update)


def test_scalar_checks_of_every_entry(lib):
    nan, inf = float("nan"), float("inf")
    for call in ENTRIES:
        assert call(lib, params=None) == BAD
        assert call(lib, params=_p(mass=0.0)) == BAD
        for bad in (dict(B=-1), dict(K=0), dict(C=0), dict(C=pt.MAX_C + 1), dict(sigma=-0.1), dict(sigma=nan), dict(sigma=inf),
                    dict(sigma=-inf)):
            assert call(lib, **bad) == BAD, (call.__name__, bad)
            assert lib.fg_last_error().decode().startswith("fg_"), bad
        assert call(lib, B=0) == OK                                   # an empty batch: nothing launched, nothing looked at
    for call in (_candidates, _update):                                # any N up to 2^12 - beyond it the stream code's field ends
        assert call(lib, N=pt.MAX_N + 1) == BAD and "2^12" in lib.fg_last_error().decode()
        assert call(lib, N=0) == BAD
    assert _sampled(lib, N=pt.MAX_N + 1) == UNSUPPORTED               # (the returns kernels' agent counts come first)
    assert _sampled(lib, N=5) == UNSUPPORTED
    assert _sampled(lib, gamma=1.5) == BAD and _sampled(lib, params=_p(u_noise=0.1)) == BAD
    assert _sampled(lib, B=70000, C=70000) == BAD


def test_pointer_checks(lib):
    for k in ("pos_x", "pos_y", "vel_x", "vel_y", "ideal_shape", "ideal_vel", "step", "mean", "ret"):
        assert _sampled(lib, **{k: None}) == BAD and "a required pointer is NULL" in lib.fg_last_error().decode(), k
    for k, v in (("mean", P + 4), ("ideal_shape", P + 4), ("pos_x", P + 2), ("ret", P + 2), ("indiv_ret", P + 1), ("steps", P + 2)):
        assert _sampled(lib, **{k: v}) == ALIGN, k
    assert _candidates(lib, act=None) == BAD
    assert _candidates(lib, act=FAR + 4) == ALIGN and _candidates(lib, mean=P + 4) == ALIGN
    for k in ("ret", "mean_in", "mean_out"):
        assert _update(lib, **{k: None}) == BAD and "a required pointer is NULL" in lib.fg_last_error().decode(), k
    for k, v in (("ret", P + 2), ("mean_in", FAR + 4), ("mean_out", 2 * FAR + 4), ("act", 3 * FAR + 4)):
        assert _update(lib, **{k: v}) == ALIGN, k


def test_update_checks(lib):
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        assert _update(lib, lam=lam) == BAD and "lambda" in lib.fg_last_error().decode(), lam
    for shift in (2, -1):
        assert _update(lib, shift=shift) == BAD and "shift" in lib.fg_last_error().decode()
    B, N, K = 4, 9, 5
    nbytes = K * B * N * 8
    for out in (FAR, FAR + 8, FAR + nbytes - 8, FAR - nbytes + 8, FAR - 8):
        assert _update(lib, mean_in=FAR, mean_out=out) == BAD, out - FAR
        assert "must not overlap" in lib.fg_last_error().decode()
    # the outputs are written while other threads read the inputs: each output apart from each input and from the other
    ret_bytes, act_bytes = 3 * B * N * 4, B * N * 8
    for bad in (dict(act=FAR), dict(act=FAR + nbytes - 8), dict(act=FAR - act_bytes + 8),               # act_out on mean_in
                dict(act=P), dict(act=P + ret_bytes - 8),                                                 # ... on ret
                dict(act=2 * FAR), dict(act=2 * FAR + nbytes - 8),                                        # ... on mean_out
                dict(mean_out=P), dict(mean_out=P + ret_bytes - 8), dict(mean_out=P - nbytes + 8)):       # mean_out on ret
        assert _update(lib, **bad) == BAD, bad
        assert "must not overlap ret, mean_in or each other" in lib.fg_last_error().decode(), bad
    # (adjacent buffers - the first addresses that do not overlap - are launched by tests/test_gpu_planner.py)


# ---- MPPIPlanner on a stand-in env ----
def _standin(path="fused", mode=0, B=6, N=3):
    world = types.SimpleNamespace(device=torch.device("cpu"))
    return types.SimpleNamespace(world=world, num_envs=B, num_agents=N, shared_reward=True, returns_path=lambda: path,
                                 _action_mode=lambda: mode, scenario=types.SimpleNamespace(_seed=1))


def test_planner_path_follows_returns_path():
    assert MPPIPlanner(_standin("fused"), 5, 4, 0.5, 1.0).path() == "fused"
    assert MPPIPlanner(_standin("replay"), 5, 4, 0.5, 1.0).path() == "materialised"


def test_planner_refuses_discrete_actions_and_bad_scalars():
    for mode in (_native.FG_ACT_ONEHOT5, _native.FG_ACT_INDEX, _native.FG_ACT_ARGMAX):
        with pytest.raises(ValueError, match="continuous"):
            MPPIPlanner(_standin(mode=mode), 5, 4, 0.5, 1.0)
    good = dict(horizon=5, candidates=4, sigma=0.5, lam=1.0)
    for bad in (dict(horizon=0), dict(horizon=2.5), dict(candidates=0), dict(candidates=pt.MAX_C + 1), dict(candidates=True),
                dict(sigma=-0.1), dict(sigma=float("nan")), dict(sigma="1"), dict(lam=0.0), dict(lam=float("inf")),
                dict(gamma=1.5), dict(gamma=-0.1), dict(clip=float("nan")), dict(noise_offset=-1), dict(noise_offset=1 << 64),
                dict(noise_offset=0.5)):
        with pytest.raises(ValueError):
            MPPIPlanner(_standin(), **dict(good, **bad))
    with pytest.raises(ValueError):
        MPPIPlanner(_standin(N=pt.MAX_N + 1), **good)
    pl = MPPIPlanner(_standin(), **good)
    assert tuple(pl.mean.shape) == (5, 6, 3, 2) and pl.mean.dtype == torch.float32 and not pl.mean.any()
    for name, v in (("sigma", -1.0), ("lam", 0.0), ("clip", float("nan")), ("gamma", 2.0)):    # read at every call
        old = getattr(pl, name)
        setattr(pl, name, v)
        with pytest.raises(ValueError, match=name):
            pl.plan()
        setattr(pl, name, old)


def test_planner_advances_its_offset_swaps_its_buffers_and_resets():
    K, C = 5, 4
    pl = MPPIPlanner(_standin(), K, C, 0.5, 1.0, noise_offset=2 ** 64 - 3)
    seen = []

    def score(off, sigma, gamma, clip):
        seen.append(("score", off, sigma, gamma, clip))
        r = torch.zeros((C, 6, 3))
        return r, {"individual_return": r, "steps": torch.zeros(6, dtype=torch.int32)}

    def update(off, sigma, clip, lam, returns, shift):
        seen.append(("update", off, sigma, clip, lam, shift))
        pl._spare.fill_(float(len(seen)))
        return torch.zeros((6, 3, 2))
    pl._score, pl._update = score, update
    first, spare = pl.mean, pl._spare
    action, info = pl.plan()
    assert set(info) == {"returns", "individual_return", "steps", "noise_offset"} and info["noise_offset"] == 2 ** 64 - 3
    assert tuple(action.shape) == (6, 3, 2)
    assert pl.mean is spare and pl._spare is first and float(pl.mean[0, 0, 0, 0]) == 2.0
    assert pl.noise_offset == (2 ** 64 - 3 + K) % 2 ** 64 == K - 3          # the 64-bit sum wraps
    pl.sigma, pl.lam, pl.clip = 0.25, 3.0, 0.0
    pl.plan(shift=False)
    assert pl.noise_offset == 2 * K - 3
    assert seen == [("score", 2 ** 64 - 3, 0.5, 1.0, 1.0), ("update", 2 ** 64 - 3, 0.5, 1.0, 1.0, True),
                    ("score", K - 3, 0.25, 1.0, 0.0), ("update", K - 3, 0.25, 0.0, 3.0, False)]
    pl.reset(torch.tensor([True, False, False, False, False, True]))
    assert not pl.mean[:, 0].any() and not pl.mean[:, 5].any() and pl.mean[:, 1:5].all()
    pl.reset()
    assert not pl.mean.any()
    with pytest.raises(ValueError):
        pl.reset(torch.ones(5, dtype=torch.bool))


# ---- the stream code ----
def test_the_planner_stream_collides_with_no_other():
    """Counter word 1 of the planner is 0x40000000 | c << 12 | i: with i < 2^12 and c < 2^17 the fields fill bits 0 .. 28, so the
    top three bits are 010 for every (c, i).  Every other stream's code keeps its own top bits for every index below 2^29:
    000 reset / landmarks, 001 obstacles, 011 Gumbel, 100 motor, 101 actor, 110 communication, 111 the ideal velocity."""
    corners = [(c, i) for c in (0, 1, pt.MAX_C - 1) for i in (0, 1, pt.MAX_N - 1)]
    mine = {pt.plan_code(c, i) for c, i in corners}
    assert len(mine) == len(corners)                                   # (c, i) -> code is one to one at the corners
    assert {code >> 29 for code in mine} == {0b010}
    assert pt.plan_code(pt.MAX_C - 1, pt.MAX_N - 1) == 0x5FFFFFFF      # the fields end exactly below bit 29
    idx = (0, 1, pt.MAX_N - 1, (1 << 29) - 1)
    tops = {}
    for name, code in cr.STREAM_CODES.items():
        args = [(i, q) for i in idx[:3] for q in (0, 1, 2)] if name == "comm_noise" else [(i,) for i in idx]
        if name == "hd_ivel":
            args = [()]
        tops[name] = {(code(*a) & 0xFFFFFFFF) >> 29 for a in args}
    tops["gumbel"] = {pt.GUMBEL_CODE(i, q) >> 29 for i in idx[:3] for q in (0, 1)}
    for name, t in tops.items():
        assert 0b010 not in t, (name, t)
    assert tops["gumbel"] == {0b011} and tops["motor_noise"] == {0b100} and tops["actor_noise"] == {0b101}
    assert tops["comm_noise"] == {0b110} and tops["hd_ivel"] == {0b111}


def test_numpy_draws_are_a_function_of_every_argument():
    base = pt.unit_draws(cr.SEED, 3, 3, 2, 2, 3, 2 ** 32 - 1)[0]
    assert base.shape == (3, 2, 2, 3, 2) and np.isfinite(base).all()
    assert len(np.unique(base.round(12))) == base.size                 # no two of (c, k, b, i, component) coincide
    assert np.array_equal(pt.unit_draws(cr.SEED, 3, 3, 2, 2, 3, 2 ** 32)[0][:, 0], base[:, 1])     # step 1 carried into the high word
    assert np.array_equal(pt.unit_draws(cr.SEED, 4, 3, 2, 1, 3, 2 ** 32 - 1)[0][:, :, 0], base[:, :, 1])   # env = base + b
    assert not np.array_equal(pt.unit_draws(cr.SEED ^ (1 << 40), 3, 3, 2, 2, 3, 2 ** 32 - 1)[0], base)      # the seed's high word


# ---- the inputs of the GPU test "a small lambda picks the best candidate" ----
def test_the_pick_tests_runner_up_gaps():
    """At most 1 % of the (env, agent) rows have a runner-up within 150 lam of the best return (fp64 oracle, NumPy candidates):
    elsewhere every other weight is below exp(-150), which is zero in fp32 (the smallest denormal is 2^-149 = exp(-103.3)), with
    room for the fp32 returns' own error (rt.F32_ORACLE_BOUND x |R| < 1e-4 << 46 lam).  No collision count of the inputs is
    within rt.F32_MARGIN of flipping, so the fp32 launch ranks the candidates as the oracle does."""
    d = pt.PICK
    best, gap, margin = pt.pick_oracle()
    rows = np.repeat(gap < pt.GAP_FACTOR * d["lam"], d["N"])           # the shared return: one gap per env, N rows each
    print("gaps: min %.4g  median %.4g  (150 lam = %.4g);  excluded rows %d of %d;  smallest collision margin %.3g"
          % (gap.min(), np.median(gap), pt.GAP_FACTOR * d["lam"], rows.sum(), rows.size, margin.min()))
    assert rows.mean() <= 0.01
    assert (margin > rt.F32_MARGIN).all()
    assert len(set(best.tolist())) > 2                                 # the best candidate is not the same everywhere
