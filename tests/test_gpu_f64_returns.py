"""returns_kernel in the fp64 parity build (csrc/formation_hip_f64.hip: fg64_rollout_hd_returns, the SAME kernel source as the
product's `fg_rollout_hd_returns` with real = double, at the product's lane group and workgroup per agent count) against
`rt.oracle_returns`: the fp64 oracle stepped K times per candidate, the discounted sum and the counting rule written out in NumPy
(tests/returns_testlib.py; tests/test_returns_cpu.py holds that reference to the golden fixtures and shows its teeth first).

What the fp32 tests cannot show, because their reference is another fp32 kernel of this library and the recurrence restated in its
order: that the step the returns kernel copied is the reference's at the agent counts only it and its fp32 siblings run, that the
recurrence, the counting rule, the pair index, the two-register action prefetch and the whole-wave early exit are the RIGHT ones.

Bound: 1e-9 max(1, |R|) (rt.F64_BOUND), the bound of the pipelined rollout's fp64 free run - per-step errors measured there are
<= 7e-12 and a return sums at most 25 of them (hd_n3_done: 100, of 3 agents that seldom touch).  A property of fp64 arithmetic, not
tuned to this kernel.  Measured maxima: profiles/returns_parity.md.  Every case is one launch of a few thousand threads at most."""
import numpy as np
import pytest

from tests import returns_testlib as rt

pytestmark = pytest.mark.gpu

FIXTURES = ["hd_n3", "hd_n3_done", "hd_n4", "hd_n9", "hd_n9_crowd", "hd_n9_constants", "hd_n16_crowd", "hd_n27", "hd_n27_crowd",
            "hd_n27_constants"]


def _compare(got, want, what):
    """`got` = returns64's dict against `want` = oracle_returns' tuple: steps exactly, both returns within the bound on every
    pair (the callers hold the margins), everything finite - nothing of the NaN / -1 fill left.  Returns the largest relative errors."""
    shared, indiv, steps, margin = want
    assert got["steps"].dtype == np.int32 and got["steps"].tolist() == steps.tolist(), (what, got["steps"], steps)
    assert np.isfinite(got["ret"]).all() and np.isfinite(got["indiv"]).all(), what
    assert (margin > 1e-9).all(), (what, margin.min())                 # no collision count on its threshold: nothing is left out
    err = {}
    for k, ref in (("ret", shared), ("indiv", indiv)):
        assert got[k].shape == ref.shape and got[k].dtype == np.float64
        rel = np.abs(got[k] - ref) / np.maximum(1.0, np.abs(ref))
        err[k] = float(rel.max())
    print("%-44s shared %.3g  indiv %.3g  (x max(1, |R|)); smallest margin %.3g" % (what, err["ret"], err["indiv"], margin.min()))
    assert err["ret"] <= rt.F64_BOUND and err["indiv"] <= rt.F64_BOUND, (what, err)
    return err


@pytest.mark.parametrize("gamma", [1.0, 0.97])
@pytest.mark.parametrize("name", FIXTURES)
def test_f64_returns_kernel_free_runs_on_the_reference_fixtures(golden, name, gamma):
    """Three candidates over the fixture's whole horizon in ONE launch: the fixture's own actions, and two of seeded U(-1, 1)
    values rounded through fp32.  At gamma = 1 the first is also the plain sum of the REFERENCE's recorded rewards over the
    counted steps (the episode ends inside the horizon in hd_n3_done: step 100 of 102, hd_n9_constants: 7 of 12, and
    hd_n27_constants: 5 of 8)."""
    from tests import f64_parity
    g = golden(name)
    T, B, N = g["acts"].shape[:3]
    P = rt.fixture_params(name, g)
    rs = np.random.RandomState(4000 + N + T)
    acts = np.concatenate([np.asarray(g["acts"], dtype=np.float64)[None],
                           rs.uniform(-1, 1, (2, T, B, N, 2)).astype(np.float32).astype(np.float64)])
    state = rt.fixture_state(g)
    want = rt.oracle_returns(state, acts, gamma, P)
    got = f64_parity.returns64(state["pos"], state["vel"], state["ideal_shape"], state["ideal_vel"], state["step"], acts, gamma,
                               params=None if P is None else f64_parity.params_of(P))
    _compare(got, want, "%s gamma %g" % (name, gamma))
    steps, shared, indiv = rt.fixture_sums(g)
    assert got["steps"].tolist() == steps.tolist()
    if gamma == 1.0:
        for k, ref in (("ret", shared), ("indiv", indiv)):
            assert (np.abs(got[k][0] - ref) <= rt.F64_BOUND * np.maximum(1.0, np.abs(ref))).all(), (name, k)


@pytest.mark.parametrize("gamma", rt.F64_GAMMAS)
@pytest.mark.parametrize("N,B,C,K", rt.F64_MAIN + rt.F64_EDGES)
def test_f64_returns_kernel_against_the_oracle(N, B, C, K, gamma):
    """Every agent count of the kernel at the crowded states and mixed episode phases of the fp32 tests, an odd K = 7 and
    gamma = 0, 0.5, 1; at 3 and 27 agents K = 1, 2, 3, one pair more than a workgroup, and C = 32 at 3 agents - two whole waves
    that leave the loop after the first iteration beside waves that run all K (rt.F64_EDGES)."""
    from tests import f64_parity
    pairs = 256 // {3: 4, 27: 32}.get(N, 64)                          # per workgroup, where the edge cases count on it
    if (N, B, C, K) in ((3, 5, 13, K), (27, 5, 5, K)):
        assert (B * C) % pairs == 1
    state, acts = rt.oracle_state(B, N, K), rt.oracle_candidates(C, K, B, N)
    want = rt.oracle_returns(state, acts, gamma)
    assert want[2].tolist() == rt.expected_steps(rt.phases(B, K, 100), K, 100).tolist()
    if (N, B, C) == (3, 5, 32):
        assert pairs == 64 and want[2][2] == 1 and (want[2][[1, 3, 4]] == K).all()       # env 2 = pairs 64 ... 95 = waves 4 and 5
    got = f64_parity.returns64(state["pos"], state["vel"], state["ideal_shape"], state["ideal_vel"], state["step"], acts, gamma)
    _compare(got, want, "N %d B %d C %d K %d gamma %g" % (N, B, C, K, gamma))
