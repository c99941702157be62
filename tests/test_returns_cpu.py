"""CPU checks of `fg_rollout_hd_returns` / `fg_describe_returns_launch` and of `MultiAgentEnv.returns_path`: the symbols, every
argument check of the two entries with its status and message (and their order), the dry run's instantiation and grid for the
eight agent counts, the path decision on stand-in worlds, and the condition the GPU tests' inputs must meet (contacts in the
crowded start states) - computed on the CPU from the seeds the GPU tests use.  No device is touched."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from formation_gym import _native, load_scenario
from formation_gym.environment import MultiAgentEnv
from oracle import formation_oracle as O
from tests import returns_testlib as rt
from tests.actor_testlib import ROOT, params as _params

P = 4096                                                   # a stand-in address: only NULL-ness and alignment are looked at
OK, BAD, UNSUPPORTED, ALIGN = _native.FG_OK, _native.FG_ERR_BAD_ARG, _native.FG_ERR_UNSUPPORTED_N, _native.FG_ERR_ALIGNMENT
WHO = "fg_rollout_hd_returns: "
POINTERS = ("pos_x", "pos_y", "vel_x", "vel_y", "ideal_shape", "ideal_vel", "step", "act", "ret", "indiv_ret", "steps")


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def _call(lib, dry=False, params="default", B=4, N=9, K=5, C=3, gamma=0.9, text="buffer", **pointers):
    """(status, fg_last_error(), text) of fg_rollout_hd_returns - of its dry run when `dry` - on stand-in pointers; `params`: None
    or keyword arguments over the defaults."""
    assert set(pointers) <= set(POINTERS)
    p = None if params is None else _params()
    for k, v in ({} if params in (None, "default") else params).items():
        setattr(p, k, v)
    if dry:
        buf = ctypes.create_string_buffer(256) if text == "buffer" else None
        rc = lib.fg_describe_returns_launch(p, B, N, K, C, buf, 256)
        return rc, lib.fg_last_error().decode(), buf.value.decode() if buf is not None else ""
    rc = lib.fg_rollout_hd_returns(p, B, N, K, C, gamma, *[pointers.get(k, P) for k in POINTERS], None)
    return rc, lib.fg_last_error().decode(), ""


def test_symbols_are_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "formation_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("fg_rollout_hd_returns", "fg_describe_returns_launch"):
        assert hasattr(lib, name) and name in _native.SIGNATURES and ("int %s(" % name) in header and name in doc, name
    assert lib.fg_abi_version() == _native.ABI_VERSION == 8           # entries added, no struct changed


# (what is wrong with the call, status, fg_last_error()); the checks both entries make, in the order in which they make them
SHARED_BAD_CALLS = [
    (dict(params=None), BAD, "params is NULL"),
    (dict(params={"mass": 0.0}), BAD, "params: mass, contact_margin and dt must be > 0"),
    (dict(params={"dist_min": 0.0}), BAD, "params: dist_min must be > 0"),
    (dict(B=-1), BAD, WHO + "B >= 0, K >= 1 and C >= 1 required"),
    (dict(K=0), BAD, WHO + "B >= 0, K >= 1 and C >= 1 required"),
    (dict(C=0), BAD, WHO + "B >= 0, K >= 1 and C >= 1 required"),
    (dict(B=0, C=-2), BAD, WHO + "B >= 0, K >= 1 and C >= 1 required"),
    (dict(params={"num_walls": 1}), BAD, WHO + "World options, per-agent properties and communication are not supported"),
    (dict(params={"u_noise": 0.1}), BAD, WHO + "World options, per-agent properties and communication are not supported"),
    (dict(params={"max_speed": 0.7}), BAD, WHO + "World options, per-agent properties and communication are not supported"),
    (dict(params={"accel": 3.0}), BAD, WHO + "World options, per-agent properties and communication are not supported"),
    (dict(params={"agent_props": P}), BAD, WHO + "World options, per-agent properties and communication are not supported"),
    (dict(params={"comm_state": P}), BAD, WHO + "World options, per-agent properties and communication are not supported"),
    (dict(N=5), UNSUPPORTED, WHO + "N must be 3, 4, 8, 9, 16, 25, 27 or 32"),
    (dict(N=10), UNSUPPORTED, WHO + "N must be 3, 4, 8, 9, 16, 25, 27 or 32"),
    (dict(N=64), UNSUPPORTED, WHO + "N must be 3, 4, 8, 9, 16, 25, 27 or 32"),
    (dict(N=81), UNSUPPORTED, WHO + "N must be 3, 4, 8, 9, 16, 25, 27 or 32"),
    (dict(B=70000, C=70000), BAD, WHO + "B * C must be below 2^31"),
    # the order
    (dict(params={"mass": 0.0}, B=-1, N=5), BAD, "params: mass, contact_margin and dt must be > 0"),
    (dict(B=-1, N=5, params={"u_noise": 0.1}), BAD, WHO + "B >= 0, K >= 1 and C >= 1 required"),
    (dict(params={"u_noise": 0.1}, N=5), BAD, WHO + "World options, per-agent properties and communication are not supported"),
    (dict(N=5, B=70000, C=70000), UNSUPPORTED, WHO + "N must be 3, 4, 8, 9, 16, 25, 27 or 32"),
    (dict(B=0, N=5), UNSUPPORTED, WHO + "N must be 3, 4, 8, 9, 16, 25, 27 or 32"),
]
# ... and those of the launching entry alone: gamma behind the counts, the buffers behind everything else
GAMMA = WHO + "gamma must be a finite number in [0, 1]"
NULL = WHO + "a required pointer is NULL"
ALIGNED = WHO + "act/ideal_shape/ideal_vel must be 8-byte, the other buffers 4-byte aligned"
ENTRY_BAD_CALLS = [
    (dict(gamma=1.5), BAD, GAMMA),
    (dict(gamma=-0.01), BAD, GAMMA),
    (dict(gamma=float("nan")), BAD, GAMMA),
    (dict(gamma=float("inf")), BAD, GAMMA),
    (dict(gamma=1.5, K=0), BAD, WHO + "B >= 0, K >= 1 and C >= 1 required"),
    (dict(gamma=1.5, params={"u_noise": 0.1}, N=5), BAD, GAMMA),
    (dict(gamma=1.5, B=0), BAD, GAMMA),
] + [(dict(**{k: None}), BAD, NULL) for k in POINTERS if k not in ("indiv_ret", "steps")] + [
    (dict(act=P + 4), ALIGN, ALIGNED),
    (dict(ideal_shape=P + 4), ALIGN, ALIGNED),
    (dict(ideal_vel=P + 4), ALIGN, ALIGNED),
    (dict(pos_x=P + 2), ALIGN, ALIGNED),
    (dict(vel_y=P + 1), ALIGN, ALIGNED),
    (dict(step=P + 2), ALIGN, ALIGNED),
    (dict(ret=P + 2), ALIGN, ALIGNED),
    (dict(indiv_ret=P + 2), ALIGN, ALIGNED),
    (dict(steps=P + 3), ALIGN, ALIGNED),
    (dict(pos_x=None, act=P + 4), BAD, NULL),
    (dict(N=5, pos_x=None), UNSUPPORTED, WHO + "N must be 3, 4, 8, 9, 16, 25, 27 or 32"),
]


@pytest.mark.parametrize("dry", [False, True])
def test_shared_argument_checks(lib, dry):
    for wrong, status, message in SHARED_BAD_CALLS:
        rc, err, text = _call(lib, dry, **wrong)
        assert (rc, err) == (status, message), (wrong, rc, err)
        assert text == ""


def test_entry_argument_checks(lib):
    for wrong, status, message in ENTRY_BAD_CALLS:
        rc, err, _ = _call(lib, False, **wrong)
        assert (rc, err) == (status, message), (wrong, rc, err)
    rc, err, _ = _call(lib, True, text=None)
    assert (rc, err) == (BAD, "fg_describe_returns_launch: out buffer required")


def test_an_empty_batch_is_ok_without_a_launch(lib):
    assert _call(lib, False, B=0, **{k: None for k in POINTERS})[0] == OK          # NULL buffers allowed, nothing launched
    assert _call(lib, True, B=0)[::2] == (OK, "")


@pytest.mark.parametrize("N", rt.FUSED_N)
def test_describe_names_the_instantiation_and_a_grid_that_covers_the_pairs(lib, N):
    G = {3: 4, 4: 4, 8: 8, 9: 16, 16: 16, 25: 32, 27: 32, 32: 32}[N]          # the lane group of step_kernel and the producers
    for B, C in ((5, 7), (1, 1), (1, 4096), (4096, 8), (16384, 16), (1, 130)):
        rc, err, text = _call(lib, True, B=B, N=N, K=20, C=C)
        assert rc == OK, err
        m = re.fullmatch(r"returns_kernel<(\d+),(\d+),(\d+)> grid (\d+) block (\d+) lds (\d+); ", text)
        assert m, text
        n, g, t, grid, block, lds = map(int, m.groups())
        assert (n, g) == (N, G) and t == block and t % 64 == 0 and 64 % g == 0
        pairs = t // g                                                              # per workgroup
        assert (grid - 1) * pairs < B * C <= grid * pairs, (text, B, C)
        assert lds == pairs * 6 * ((N + 3) // 4 * 4) * 4 <= 64 * 1024             # QX QY PX PY SX SY per pair, nothing else


def test_unsupported_agent_counts(lib):
    for N in (5, 10, 64, 81):
        for dry in (False, True):
            assert _call(lib, dry, N=N)[0] == UNSUPPORTED, (N, dry)


# ---- MultiAgentEnv.returns_path on stand-in envs: the scenario object and a world that answers what `Scenario.params` asks ----
def _standin(name, N, silent=True, **options):
    sc = load_scenario(name)
    sc._seed = 1

    def native_params(**kw):
        p = _params(dist_min=0.06, collide_thresh=kw.get("collide_thresh", 0.03))
        for k, v in options.items():
            setattr(p, k, v)
        return p
    world = types.SimpleNamespace(agents=[types.SimpleNamespace(size=0.03) for _ in range(N)], num_envs=64, dim_c=2,
                                  device=torch.device("cpu"), any_non_silent=lambda: not silent, native_params=native_params)
    return types.SimpleNamespace(scenario=sc, world=world, post_step_callback=None, num_agents=N,
                                 RETURNS_FUSED_N=MultiAgentEnv.RETURNS_FUSED_N)


def test_returns_path():
    path = MultiAgentEnv.returns_path
    for N in rt.FUSED_N:
        assert path(_standin("formation_hd_env", N)) == "fused", N
    assert MultiAgentEnv.RETURNS_FUSED_N == rt.FUSED_N
    for N in (5, 10, 64, 81):
        assert path(_standin("formation_hd_env", N)) == "replay", N
    for option in (dict(num_walls=1), dict(u_noise=0.1), dict(max_speed=0.7), dict(accel=3.0), dict(agent_props=P)):
        assert path(_standin("formation_hd_env", 9, **option)) == "replay", option
    assert path(_standin("formation_hd_env", 9, silent=False)) == "replay"         # the communication block
    cb = _standin("formation_hd_env", 9)
    cb.post_step_callback = lambda world: None                                     # a host function after every step
    assert path(cb) == "replay"
    scripted = _standin("formation_hd_env", 9)

    def refuse(**kw):
        raise NotImplementedError("scripted agents")
    scripted.world.native_params = refuse
    assert path(scripted) == "replay"
    assert path(_standin("basic_formation_env", 3)) == "replay"                    # a landmark scenario: no returns kernel
    forced = _standin("formation_hd_env", 9)
    forced._returns_replay_only = True                                             # the GPU tests' switch
    assert path(forced) == "replay"


def test_rollout_returns_refuses_a_bad_gamma_before_anything_else():
    env = _standin("formation_hd_env", 9)
    for gamma in (1.5, -0.1, float("nan"), float("inf"), "0.9", None, True):
        with pytest.raises(ValueError, match="gamma"):
            MultiAgentEnv.rollout_returns(env, None, gamma)


# ---- the inputs of the GPU tests: their crowded states contain contacts ----
def test_the_crowded_states_of_the_gpu_tests_contain_contacts():
    """At least a quarter of the envs start with a pair closer than dist_min, for every (B, N) tests/test_gpu_returns.py builds -
    the single env of the B = 1 cases included: the contact force and the collision count are part of what is compared."""
    shapes = [(5, N) for N in rt.FUSED_N] + [(1, 3), (1, 27)]
    for B, N in shapes:
        pos, vel = rt.crowded_state(B, N)
        assert pos.shape == vel.shape == (B, N, 2) and pos.dtype == torch.float32
        hit = rt.envs_in_contact(pos)
        assert 4 * int(hit.sum()) >= B, (B, N, hit.tolist())


def test_the_phases_of_the_gpu_tests():
    K, wl = 6, 100
    ph = rt.phases(5, K, wl)
    assert rt.expected_steps(ph, K, wl).tolist() == [2, K, 1, K, K]
    assert rt.expected_steps(rt.phases(5, 1, wl), 1, wl).tolist() == [1] * 5


# ---- the fp64 reference of the returns (rt.oracle_returns): held to the golden fixtures, then its teeth at the GPU tests' inputs ----
ORACLE_FIXTURES = ["hd_n3", "hd_n3_done", "hd_n4", "hd_n9", "hd_n9_crowd", "hd_n16_crowd", "hd_n27_crowd"]


@pytest.mark.parametrize("name", ORACLE_FIXTURES)
def test_oracle_returns_sums_the_fixtures_recorded_rewards(golden, name):
    """The fixture's own actions as the single candidate, gamma = 1: the plain sum of the reference's recorded shared and
    individual rewards over the counted steps, to 1e-12 relative (the level at which tests/test_oracle_golden.py holds the oracle's
    steps), and the counted steps are what the recorded done flags say - hd_n3_done's episode ends at step 100 of 102."""
    g = golden(name)
    T, B, N = g["acts"].shape[:3]
    shared, indiv, steps, margin = rt.oracle_returns(rt.fixture_state(g), g["acts"][None], 1.0, rt.fixture_params(name, g))
    want_steps, want_shared, want_indiv = rt.fixture_sums(g)
    assert steps.dtype == np.int32 and steps.tolist() == want_steps.tolist()
    if name == "hd_n3_done":
        assert steps.tolist() == [100] and T == 102
    else:
        assert steps.tolist() == [T] * B
    for got, want in ((shared[0], want_shared), (indiv[0], want_indiv)):
        assert got.shape == (B, N)
        assert (np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), np.abs(got - want).max()
    assert margin.shape == (1, B) and (margin > 0).all()


def _per_step(state, acts, P=None):
    """(shared, indiv) [C,K,B,N] of every step of every candidate, by O.step_hd: what the mutants below accumulate wrongly"""
    C, K, B, N = acts.shape[:4]
    sh, ind = np.zeros((C, K, B, N)), np.zeros((C, K, B, N))
    for c in range(C):
        st = dict(state)
        for k in range(K):
            st, out = O.step_hd(st, acts[c, k], P)
            sh[c, k], ind[c, k] = out["shared"][:, None], out["indiv"]
    return sh, ind


def _accumulate(r, steps, gamma, d0=1.0, on_sum=False):
    """R [C,B,N] of the per-step rewards r [C,K,B,N]: R += d r, d *= gamma from d = d0 over the first steps[b] steps; on_sum:
    R = gamma R + r instead."""
    R = np.zeros(r[:, 0].shape)
    d = d0
    for k in range(r.shape[1]):
        live = (k < steps)[None, :, None]
        R = np.where(live, gamma * R + r[:, k] if on_sum else R + d * r[:, k], R)
        d *= gamma
    return R


MUTANT_FACTOR = 100.0


MUTANTS = ("discount starts at gamma", "done step not counted", "one step too many", "q decoded as c B + b",
           "last action of an odd K repeated", "gamma on the sum")


def mutant_factors(N, B, C, K):
    """{mutant: (factor, values)} at the inputs of the fp64 GPU test of N agents.  A compared value is one shared or individual
    return of a (candidate, env, agent) at one of the test's gammas (rt.F64_GAMMAS), wherever the mistake can show at all (the
    gammas and envs are named per mutant below); it moves by |mutant - reference| / max(1, |reference|).  factor: what 90 % of
    the values move by at least (their 10th percentile), in units of rt.F32_ORACLE_BOUND."""
    state, acts = rt.oracle_state(B, N, K), rt.oracle_candidates(C, K, B, N)
    sh, ind = _per_step(state, acts)
    n = rt.oracle_returns(state, acts, 1.0)[2]
    assert n.tolist() == [2, K, 1, K, K] and K % 2 == 1 and K > 1
    ends = state["step"] + n >= O.HdParams.world_length                  # [B]: the episode's end is inside the counted steps
    swapped = np.array(acts)
    swapped[:, K - 1] = swapped[:, K - 2]
    sh_sw, ind_sw = _per_step(state, swapped)
    q = np.arange(B)[None, :] * C + np.arange(C)[:, None]                # [C,B]: the launch's pair index b C + c
    cq, bq = q // B, q % B                                               # ... decoded the wrong way round
    every = np.ones(B, dtype=bool)
    moved = {name: [] for name in MUTANTS}
    for gamma in rt.F64_GAMMAS:
        ref = [rt.oracle_returns(state, acts, gamma)[i] for i in (0, 1)]
        for r, want in zip((sh, ind), ref):
            assert np.array_equal(_accumulate(r, n, gamma), want)       # the mutants below are mutants of the reference itself
        mutants = {
            # name: (its (shared, indiv), the envs [B] - or pairs [C,B] - in which it can show at this gamma)
            MUTANTS[0]: ([_accumulate(r, n, gamma, d0=gamma) for r in (sh, ind)], every & (gamma < 1)),
            MUTANTS[1]: ([_accumulate(r, n - ends, gamma) for r in (sh, ind)], ends & ((gamma > 0) | (n == 1))),
            MUTANTS[2]: ([_accumulate(r, np.minimum(K, n + 1), gamma) for r in (sh, ind)], (n < K) & (gamma > 0)),
            MUTANTS[3]: ([w[cq, bq] for w in ref], (cq != np.arange(C)[:, None]) | (bq != np.arange(B)[None, :])),
            MUTANTS[4]: ([_accumulate(r, n, gamma) for r in (sh_sw, ind_sw)], (n == K) & (gamma > 0)),
            MUTANTS[5]: ([_accumulate(r, n, gamma, on_sum=True) for r in (sh, ind)], (n > 1) & (gamma < 1)),
        }
        for name, (got, where) in mutants.items():
            where = np.broadcast_to(where if where.ndim == 2 else where[None, :], (C, B))[None, :, :, None]
            rel = np.stack([np.abs(g_ - w) / np.maximum(1.0, np.abs(w)) for g_, w in zip(got, ref)])
            moved[name].append(rel[np.broadcast_to(where, rel.shape)])
    out = {}
    for name in MUTANTS:
        values = np.concatenate(moved[name])
        assert values.size >= 2 * C * N                                  # one env's values at least
        out[name] = (float(np.percentile(values, 10, method="lower")) / rt.F32_ORACLE_BOUND, values.size)
    return out


@pytest.mark.parametrize("N,B,C,K", rt.F64_MAIN)
def test_the_mutants_of_the_recurrence_move_the_reference(N, B, C, K):
    """Six wrong returns kernels, each shown on the reference alone at the fp64 GPU test's inputs: at least 90 % of the compared
    values move by 100 x the widest tolerance any GPU test of the returns uses (rt.F32_ORACLE_BOUND, relative to max(1, |R|); the
    fp64 tests' 1e-9 is far inside it).  No tolerance of those tests can hide one of these.  (Measured: profiles/returns_parity.md)"""
    for name, (factor, values) in mutant_factors(N, B, C, K).items():
        print("N = %2d  %-34s 90 %% of %4d values move by >= %.3g x the bound" % (N, name, values, factor))
        assert factor >= MUTANT_FACTOR, (N, name, factor)


@pytest.mark.parametrize("N,B,C,K", rt.F64_MAIN + rt.F64_EDGES + [(N, 5, 7, 3) for N in rt.FUSED_N if N not in (3, 27)])
def test_the_collision_counts_of_the_gpu_tests_are_off_their_thresholds(N, B, C, K):
    """Every (candidate, env) pair of the fp64 GPU tests' inputs keeps its collision counts more than 1e-9 from flipping over the
    counted steps - the fp64 check leaves nothing out - and at least 80 % keep 1e-4: what the fp32 check against the oracle
    (tests/test_gpu_returns.py; K = 3 at every agent count) can compare."""
    margin = rt.oracle_returns(rt.oracle_state(B, N, K), rt.oracle_candidates(C, K, B, N), 1.0)[3]
    assert margin.shape == (C, B) and (margin > 1e-9).all(), margin.min()
    assert (margin > 1e-4).mean() >= 0.8, (margin > 1e-4).mean()
