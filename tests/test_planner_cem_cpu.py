"""CPU checks of the CEM planner entries (`fg_plan_candidates_std`, `fg_rollout_hd_returns_sampled_std` and its dry run,
`fg_plan_cem_update`) and of `formation_gym.CEMPlanner`: the symbols, the dry run against `fg_describe_returns_launch`, every
argument check that precedes a launch, the NumPy reference selection the GPU tests compare with, and the planner's host logic on
the stand-in env of tests/test_planner_cpu.py.  No device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from formation_gym import CEMPlanner, _native
from tests import planner_cem_testlib as ct
from tests import planner_testlib as pt
from tests import returns_testlib as rt
from tests.actor_testlib import ROOT, params as _params
from tests.test_planner_cpu import _standin

P = 4096                                                   # a stand-in address: only NULL-ness, alignment and ranges are looked at
FAR = 1 << 30                                              # ... and others far from it
OK, BAD, UNSUPPORTED, ALIGN = _native.FG_OK, _native.FG_ERR_BAD_ARG, _native.FG_ERR_UNSUPPORTED_N, _native.FG_ERR_ALIGNMENT
NEW = ("fg_plan_candidates_std", "fg_rollout_hd_returns_sampled_std", "fg_describe_returns_sampled_std_launch", "fg_plan_cem_update")


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
    assert CEMPlanner.__module__ == "formation_gym.planner"


def test_the_exported_caps_are_the_kernels():
    src = open(os.path.join(ROOT, "gym-formation_amd", "csrc", "fg_planner_kernels.hpp")).read()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))
    assert (_native.CEM_REG_C, _native.CEM_ELITE_CAP) == (const("FG_CEM_REG_C"), const("FG_CEM_ELITE_CAP"))
    assert _native.CEM_REG_C % 64 == 0 and _native.CEM_ELITE_CAP < _native.CEM_REG_C < pt.MAX_C


# ---- the dry run ----
def _describe(lib, fn, p, B, N, K, C):
    buf = ctypes.create_string_buffer(256)
    rc = getattr(lib, fn)(p, B, N, K, C, buf, 256)
    return rc, buf.value.decode()


@pytest.mark.parametrize("N", rt.FUSED_N)
def test_dry_run_is_the_returns_kernels_with_the_name_changed(lib, N):
    for B, C in ((5, 7), (1, 1), (1, 4096), (4096, 8), (16384, 16), (1, 130), (1, pt.MAX_C)):
        rc, text = _describe(lib, "fg_describe_returns_launch", _p(), B, N, 20, C)
        rc_s, text_s = _describe(lib, "fg_describe_returns_sampled_std_launch", _p(), B, N, 20, C)
        assert rc == rc_s == OK and text.startswith("returns_kernel<")
        assert text_s == text.replace("returns_kernel<", "returns_sampled_std_kernel<", 1)


def test_dry_run_status_codes(lib):
    for kw, B, N, C in ((dict(), 4, 5, 3), (dict(), 4, 81, 3), (dict(u_noise=0.1), 4, 9, 3), (dict(num_walls=1), 4, 9, 3),
                        (dict(agent_props=P), 4, 9, 3), (dict(), 70000, 9, 70000), (dict(), -1, 9, 3), (dict(), 4, 9, 0)):
        want = _describe(lib, "fg_describe_returns_launch", _p(**kw), B, N, 5, C)
        got = _describe(lib, "fg_describe_returns_sampled_std_launch", _p(**kw), B, N, 5, C)
        assert want[0] != OK and got == (want[0], ""), (kw, B, N, C)
    assert _describe(lib, "fg_describe_returns_sampled_std_launch", _p(), 1, 9, 5, pt.MAX_C + 1) == (BAD, "")
    assert "C <= 2^17" in lib.fg_last_error().decode()
    assert _describe(lib, "fg_describe_returns_sampled_std_launch", None, 1, 9, 5, 3)[0] == BAD
    assert lib.fg_describe_returns_sampled_std_launch(_p(), 1, 9, 5, 3, None, 0) == BAD
    assert "fg_describe_returns_sampled_std_launch" in lib.fg_last_error().decode()
    assert _describe(lib, "fg_describe_returns_sampled_std_launch", _p(), 0, 9, 5, 3) == (OK, "")


# ---- the argument checks that precede a launch ----
SAMPLED_PTRS = ("pos_x", "pos_y", "vel_x", "vel_y", "ideal_shape", "ideal_vel", "step", "mean", "std", "ret", "indiv_ret", "steps")


def _sampled(lib, params="default", B=4, N=9, K=5, C=3, gamma=0.9, off=7, clip=1.0, **ptrs):
    assert set(ptrs) <= set(SAMPLED_PTRS)
    p = _p() if params == "default" else params
    return lib.fg_rollout_hd_returns_sampled_std(p, B, N, K, C, gamma, off, clip, *[ptrs.get(k, P) for k in SAMPLED_PTRS], None)


def _candidates(lib, params="default", B=4, N=9, K=5, C=3, off=7, clip=1.0, mean=P, std=2 * FAR, act=FAR):
    return lib.fg_plan_candidates_std(_p() if params == "default" else params, B, N, K, C, off, clip, mean, std, act, None)


UPDATE_PTRS = dict(ret=P, mean_in=FAR, std_in=2 * FAR, mean_out=3 * FAR, std_out=4 * FAR, act=5 * FAR, elites=6 * FAR)


def _update(lib, params="default", B=4, N=9, K=5, C=3, E=2, off=7, clip=1.0, alpha=1.0, sigma_min=0.0, shift=1, **ptrs):
    assert set(ptrs) <= set(UPDATE_PTRS)
    a = dict(UPDATE_PTRS, **ptrs)
    return lib.fg_plan_cem_update(_p() if params == "default" else params, B, N, K, C, E, off, clip, alpha, sigma_min, a["ret"],
                                  a["mean_in"], a["std_in"], a["mean_out"], a["std_out"], a["act"], a["elites"], shift, None)


ENTRIES = (_sampled, _candidates, _update)


def test_scalar_checks_of_every_entry(lib):
    for call in ENTRIES:
        assert call(lib, params=None) == BAD
        assert call(lib, params=_p(mass=0.0)) == BAD
        for bad in (dict(B=-1), dict(K=0), dict(C=0), dict(C=pt.MAX_C + 1)):
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


def test_update_scalar_checks(lib):
    nan, inf = float("nan"), float("inf")
    for E in (0, 4, -1):                                               # C = 3
        assert _update(lib, E=E) == BAD and "1 <= E <= C" in lib.fg_last_error().decode(), E
    assert _update(lib, E=3, ret=None) == BAD and "NULL" in lib.fg_last_error().decode()      # E = C passes the scalar checks
    for alpha in (0.0, 1.5, nan, -0.5, inf):
        assert _update(lib, alpha=alpha) == BAD and "alpha" in lib.fg_last_error().decode(), alpha
    for sigma_min in (-1.0, inf, nan):
        assert _update(lib, sigma_min=sigma_min) == BAD and "sigma_min" in lib.fg_last_error().decode(), sigma_min
    for shift in (2, -1):
        assert _update(lib, shift=shift) == BAD and "shift" in lib.fg_last_error().decode()
    # the order of fg_plan_mppi_update: the scalars, then the empty batch, then the pointers
    assert _update(lib, E=0, B=0) == BAD and _update(lib, B=0, ret=None) == OK


def test_pointer_checks(lib):
    for k in SAMPLED_PTRS[:10]:
        assert _sampled(lib, **{k: None}) == BAD and "a required pointer is NULL" in lib.fg_last_error().decode(), k
    for k, v in (("mean", P + 4), ("std", P + 4), ("ideal_shape", P + 4), ("pos_x", P + 2), ("ret", P + 2), ("indiv_ret", P + 1),
                 ("steps", P + 2)):
        assert _sampled(lib, **{k: v}) == ALIGN, k
    for k in ("std", "act"):
        assert _candidates(lib, **{k: None}) == BAD and "a required pointer is NULL" in lib.fg_last_error().decode(), k
    for k, v in (("act", FAR + 4), ("mean", P + 4), ("std", 2 * FAR + 4)):
        assert _candidates(lib, **{k: v}) == ALIGN, k
    for k in ("ret", "mean_in", "std_in", "mean_out", "std_out"):
        assert _update(lib, **{k: None}) == BAD and "a required pointer is NULL" in lib.fg_last_error().decode(), k
    for k, v in UPDATE_PTRS.items():
        assert _update(lib, **{k: v + (2 if k in ("ret", "elites") else 4)}) == ALIGN, k


def test_update_overlap_checks(lib):
    """Every output against every input and every other output, at the first and the last overlapping byte from either side."""
    B, N, K, C, E = 4, 9, 5, 3, 2
    plan, size = K * B * N * 8, dict(ret=C * B * N * 4, act=B * N * 8, elites=E * B * N * 4)
    nbytes = lambda k: size.get(k, plan)
    outs, ins = ("mean_out", "std_out", "act", "elites"), ("ret", "mean_in", "std_in")
    pairs = [(o, i) for o in outs for i in ins] + [(o, q) for n, o in enumerate(outs) for q in outs[:n]]
    assert len(pairs) == 18
    for o, other in pairs:
        base = UPDATE_PTRS[other]
        grain = 8 if o != "elites" else 4                                      # (keep `o` aligned)
        first, last = base - nbytes(o) + grain, base + nbytes(other) - grain
        for at in (base, first, last):
            assert _update(lib, **{o: at}) == BAD, (o, other, at - base)
            assert "must not overlap ret, mean_in, std_in or each other" in lib.fg_last_error().decode(), (o, other)
    # (adjacent buffers - the first addresses that do not overlap - are launched by tests/test_gpu_planner_cem.py)


# ---- the NumPy reference selection ----
def test_reference_key_order_is_numpy_sort_on_finite_floats():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(500), rng.standard_normal(100) * 1e30, rng.standard_normal(100) * 1e-40,
                        [np.finfo(np.float32).max, -np.finfo(np.float32).max, 1.0, -1.0]]).astype(np.float32)
    by_key = x[np.argsort(ct.keys(x), kind="stable")]
    assert np.array_equal(by_key, np.sort(x))
    k = ct.keys(np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf], np.float32)).astype(np.int64)
    assert (np.diff(k) > 0).all()                                      # -0 ranks below +0, the infinities at the ends
    assert ct.keys(np.float32([np.nan])).dtype == np.uint32            # (defined for every bit pattern)


def test_reference_selection_ties_and_ends():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 4, (40, 6)).astype(np.float32)                 # heavy ties
    for E in (1, 2, 7, 39, 40):
        sel = ct.select(x, E)
        assert sel.shape == (E, 6) and sel.dtype == np.int32 and (np.diff(sel, axis=0) > 0).all()
        for j in range(6):
            order = sorted(range(40), key=lambda c: (-x[c, j], c))     # ties stable: the lower index first
            assert sel[:, j].tolist() == sorted(order[:E])
    assert np.array_equal(ct.select(x, 1)[0], x.argmax(0))             # E = 1: argmax, its lowest index
    assert np.array_equal(ct.select(x, 40), np.broadcast_to(np.arange(40, dtype=np.int32)[:, None], (40, 6)))
    z = np.array([0.0, -0.0, 0.0, -0.0], np.float32)[:, None]
    assert ct.select(z, 2)[:, 0].tolist() == [0, 2]                    # +0 above -0
    for C in (1, 2, 63, 130):
        rows = ct.pattern_rows(C, 0, 7)
        assert rows.shape == (C, 7) and rows.dtype == np.float32
        assert all(1 <= e <= C for e in ct.elite_counts(C, _native.CEM_ELITE_CAP))
    assert {_native.CEM_ELITE_CAP, _native.CEM_ELITE_CAP + 1} <= set(ct.elite_counts(_native.CEM_REG_C + 1, _native.CEM_ELITE_CAP))


# ---- CEMPlanner on the stand-in env ----
GOOD = dict(horizon=5, candidates=4, elites=2, sigma=0.5)


def test_planner_path_follows_returns_path():
    assert CEMPlanner(_standin("fused"), **GOOD).path() == "fused"
    assert CEMPlanner(_standin("replay"), **GOOD).path() == "materialised"


def test_planner_refuses_discrete_actions_and_bad_scalars():
    for mode in (_native.FG_ACT_ONEHOT5, _native.FG_ACT_INDEX, _native.FG_ACT_ARGMAX):
        with pytest.raises(ValueError, match="continuous"):
            CEMPlanner(_standin(mode=mode), **GOOD)
    for bad in (dict(horizon=0), dict(horizon=2.5), dict(candidates=0), dict(candidates=pt.MAX_C + 1), dict(candidates=True),
                dict(elites=0), dict(elites=5), dict(elites=2.0), dict(elites=True), dict(iterations=0), dict(iterations=1.5),
                dict(sigma=-0.1), dict(sigma=float("nan")), dict(sigma="1"), dict(alpha=0.0), dict(alpha=1.5),
                dict(alpha=float("nan")), dict(sigma_min=-1.0), dict(sigma_min=float("inf")), dict(gamma=1.5), dict(gamma=-0.1),
                dict(clip=float("nan")), dict(noise_offset=-1), dict(noise_offset=1 << 64), dict(noise_offset=0.5)):
        with pytest.raises(ValueError):
            CEMPlanner(_standin(), **dict(GOOD, **bad))
    with pytest.raises(ValueError):
        CEMPlanner(_standin(N=pt.MAX_N + 1), **GOOD)
    pl = CEMPlanner(_standin(), **GOOD)
    assert tuple(pl.mean.shape) == tuple(pl.std.shape) == (5, 6, 3, 2) and pl.mean.dtype == pl.std.dtype == torch.float32
    assert not pl.mean.any() and (pl.std == 0.5).all()
    for name, v in (("sigma", -1.0), ("elites", 5), ("iterations", 0), ("alpha", 0.0), ("sigma_min", -1.0), ("clip", float("nan")),
                    ("gamma", 2.0)):                                   # read at every call
        old = getattr(pl, name)
        setattr(pl, name, v)
        with pytest.raises(ValueError, match=name):
            pl.plan()
        setattr(pl, name, old)


def test_planner_iterates_advances_its_offset_swaps_its_buffers_and_resets():
    K, C, E, ITER = 5, 4, 2, 3
    pl = CEMPlanner(_standin(), K, C, E, 0.5, iterations=ITER, alpha=0.5, sigma_min=0.125, noise_offset=2 ** 64 - 7)
    seen = []

    def score(off, gamma, clip):
        seen.append(("score", off, gamma, clip, float(pl.std[0, 0, 0, 0])))
        r = torch.zeros((C, 6, 3))
        return r, {"individual_return": r, "steps": torch.zeros(6, dtype=torch.int32)}

    def update(off, clip, elites, alpha, sigma_min, returns, shift):
        seen.append(("update", off, clip, elites, alpha, sigma_min, shift))
        pl._spare.fill_(float(len(seen)))
        pl._std_spare.fill_(0.25)
        return torch.zeros((6, 3, 2)), torch.zeros((elites, 6, 3), dtype=torch.int32)
    pl._score, pl._update = score, update
    bufs = (pl.mean, pl._spare, pl.std, pl._std_spare)
    action, info = pl.plan()
    assert set(info) == {"returns", "individual_return", "steps", "std", "elites", "noise_offset"}
    assert info["noise_offset"] == 2 ** 64 - 7 and tuple(action.shape) == (6, 3, 2) and tuple(info["elites"].shape) == (E, 6, 3)
    # three swaps: the buffers have changed places, in step
    assert pl.mean is bufs[1] and pl._spare is bufs[0] and pl.std is bufs[3] and pl._std_spare is bufs[2]
    assert info["std"] is pl.std and float(pl.mean[0, 0, 0, 0]) == 6.0
    o = [(2 ** 64 - 7 + j * K) % 2 ** 64 for j in range(ITER)]
    assert o[2] == 3 and pl.noise_offset == (2 ** 64 - 7 + ITER * K) % 2 ** 64 == 8       # the 64-bit sums wrap
    assert seen == [("score", o[0], 1.0, 1.0, 0.5), ("update", o[0], 1.0, E, 0.5, 0.125, False),     # std = sigma at the start,
                    ("score", o[1], 1.0, 1.0, 0.25), ("update", o[1], 1.0, E, 0.5, 0.125, False),    # the refit std afterwards;
                    ("score", o[2], 1.0, 1.0, 0.25), ("update", o[2], 1.0, E, 0.5, 0.125, True)]     # shift: the last round only
    del seen[:]
    pl.sigma, pl.iterations, pl.clip, pl.elites = 0.75, 1, 0.0, 4
    pl.plan(shift=False)
    assert seen == [("score", 8, 1.0, 0.0, 0.75), ("update", 8, 0.0, 4, 0.5, 0.125, False)]          # std filled again
    assert pl.noise_offset == 8 + K
    pl.reset(torch.tensor([True, False, False, False, False, True]))
    assert not pl.mean[:, 0].any() and not pl.mean[:, 5].any() and pl.mean[:, 1:5].all()
    pl.reset()
    assert not pl.mean.any()
    with pytest.raises(ValueError):
        pl.reset(torch.ones(5, dtype=torch.bool))
