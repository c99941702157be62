"""`MultiAgentEnv.rollout_returns` on the GPU: the fused launch (`fg_rollout_hd_returns`, returns_kernel) and the replay route
against the reference of tests/returns_testlib.py - `env.rollout` per candidate and a Python loop of torch fp32 ops - bit for bit
(`torch.equal`), and the env left exactly where it was.  Every case is small: crowded states (tests/test_returns_cpu.py holds
them to containing contacts), envs at mixed episode phases, a handful of candidates."""
import numpy as np
import pytest
import torch

from formation_gym import _native
from tests import returns_testlib as rt

pytestmark = pytest.mark.gpu

B, C, K = 5, 7, 6


def _check(e, a, gamma, want=None, path="fused"):
    """`rollout_returns` of `e` against the reference `want` (made here when None): returns, individual returns, steps, the
    choice between the two by `shared_reward`, fresh tensors, the env untouched.  Returns the reference."""
    if want is None:
        want = rt.reference(e, a, gamma)
    shared, own, steps = want
    assert e.returns_path() == path
    before = rt.env_facts(e)
    ret, info = e.rollout_returns(a, gamma)
    shape = (a.shape[0], e.num_envs, e.num_agents)
    assert tuple(ret.shape) == tuple(info["individual_return"].shape) == shape and ret.dtype == torch.float32
    assert info["steps"].dtype == torch.int32 and tuple(info["steps"].shape) == (e.num_envs,)
    assert torch.equal(info["steps"], steps)
    assert torch.equal(info["steps"].cpu(), rt.expected_steps(before[0]["step_count"].cpu(), int(a.shape[1]), int(e.world.world_length)))
    assert torch.equal(info["individual_return"], own)
    assert torch.equal(ret, shared if e.shared_reward else own)
    assert torch.isfinite(ret).all()
    rt.assert_same_facts(before, rt.env_facts(e))
    return want


def _replay(e):
    e._returns_replay_only = True                      # the private switch: the replay route on a fused shape
    return e


@pytest.mark.parametrize("gamma", [1.0, 0.97])
@pytest.mark.parametrize("N", rt.FUSED_N)
def test_fused_and_replay_equal_the_reference(N, gamma):
    e = rt.env(N, B, K)
    a = rt.candidates(C, K, B, N)
    want = _check(e, a, gamma)
    assert want[2].tolist() == [2, K, 1, K, K]         # the phases: an episode ends at step 2, at step K, has ended; two run on
    if gamma == 1.0:                                   # discounting shows: the two gammas differ where more than one step counts
        other = rt.reference(e, a, 0.97)
        assert not torch.equal(other[0][:, 1], want[0][:, 1]) and torch.equal(other[0][:, 2], want[0][:, 2])
    _check(_replay(e), a, gamma, want, path="replay")


@pytest.mark.parametrize("shared_reward", [True, False])
def test_shared_reward_chooses_the_return(shared_reward):
    e = rt.env(9, B, K)
    e.shared_reward = shared_reward
    a = rt.candidates(C, K, B, 9)
    want = _check(e, a, 0.97)
    assert not torch.equal(want[0], want[1])
    _check(_replay(e), a, 0.97, want, path="replay")


# pairs per workgroup: 64 at 3 agents, 8 at 27
@pytest.mark.parametrize("N,shape", [(N, s) for N in (3, 27) for s in ("C=1", "K=1", "B=1,C=130", "one more than a workgroup")])
def test_geometry_edges(N, shape):
    b, c, k = {"C=1": (B, 1, K), "K=1": (B, C, 1), "B=1,C=130": (1, 130, K),
               "one more than a workgroup": (5, 13, K) if N == 3 else (5, 5, K)}[shape]
    if shape == "one more than a workgroup":
        assert (b * c) % (64 if N == 3 else 8) == 1
    e = rt.env(N, b, k)
    _check(e, rt.candidates(c, k, b, N), 0.97)


@pytest.mark.parametrize("route", ["fused", "replay"])
def test_nothing_moved_and_a_following_rollout_is_the_twins(route):
    """After the call - the replay with `auto_reset` on and the device RNG counter - nothing of the env has moved, and a following
    `rollout` (auto-reset draws included) gives the bits of a twin env that never made the call."""
    N = 9
    e, twin = rt.env(N, B, K), rt.env(N, B, K)
    for x in (e, twin):
        x.auto_reset = True
        if route == "replay":
            x.use_device_rng_counter(True)
    if route == "replay":
        _replay(e)
    a = rt.candidates(C, K, B, N)
    before = rt.env_facts(e)
    e.rollout_returns(a, 0.97)
    rt.assert_same_facts(before, rt.env_facts(e))
    assert e.auto_reset is True
    nxt = rt.candidates(1, K, B, N, seed=rt.SEED + 1)[0]
    got, ref = e.rollout(nxt, out=False), twin.rollout(nxt, out=False)
    for x, y in zip(got[:3], ref[:3]):
        assert torch.equal(x, y)
    assert torch.equal(got[3]["individual_reward"], ref[3]["individual_reward"])
    assert got[2].any()                                # episodes ended inside it: the reset draws were the twin's
    rt.assert_same_facts(rt.env_facts(e), rt.env_facts(twin))


def test_index_actions_are_decoded_in_one_launch():
    N = 3
    e = rt.env(N, B, K)
    e.discrete_action_input = True
    assert e._action_mode() == _native.FG_ACT_INDEX
    a = rt.candidates(C, K, B, N, mode="index")
    want = _check(e, a, 0.97)
    _check(_replay(e), a, 0.97, want, path="replay")


def test_replay_where_no_kernel_exists():
    from formation_gym.core import Wall
    e = rt.env(9, B, K)
    e.world.walls = [Wall("V", -0.3, (-1.0, 1.0), 0.1), Wall("H", 0.25, (-0.5, 0.5), 0.2)]
    _check(e, rt.candidates(C, K, B, 9), 0.97, path="replay")
    e = rt.env(3, B, K, name="basic_formation_env")
    _check(e, rt.candidates(C, K, B, 3), 0.97, path="replay")


@pytest.mark.parametrize("route", ["fused", "replay"])
def test_bad_arguments_raise_and_launch_nothing(route):
    N = 9
    e = rt.env(N, B, K)
    if route == "replay":
        _replay(e)
    before = rt.env_facts(e)
    good = rt.candidates(C, K, B, N)
    for bad in (good[:, :, :, :, :1], good[:, :, :4], good[0], good[:0], good[:, :0], good.cpu().numpy()):
        with pytest.raises(ValueError):
            e.rollout_returns(bad)
    with pytest.raises(ValueError):
        e.rollout_returns(good, gamma=1.5)
    rt.assert_same_facts(before, rt.env_facts(e))


# ---- the shapes no case above runs: the same `_check`, both routes, bit for bit ----
@pytest.mark.parametrize("k", [2, 3, 5, 7])
@pytest.mark.parametrize("N", [3, 9, 27])
def test_short_and_odd_horizons(N, k):
    """K = 2: the second fetch of the two-register action prefetch is already the clamped one; an odd K: the loop unrolled by two
    ends on an unpaired step, whose prefetch re-reads the last action."""
    e = rt.env(N, B, k)
    a = rt.candidates(C, k, B, N)
    want = _check(e, a, 0.97)
    assert want[2].tolist() == [2, k, 1, k, k]
    _check(_replay(e), a, 0.97, want, path="replay")


@pytest.mark.parametrize("N", [3, 9, 27])
def test_gamma_zero_returns_the_first_steps_reward(N):
    """gamma = 0: d_1 = 0 and every later term is a signed zero, so the return has the bits of the first counted step's reward -
    the one-step launch's return."""
    e = rt.env(N, B, K)
    a = rt.candidates(C, K, B, N)
    want = _check(e, a, 0.0)
    first = rt.reference(e, a[:, :1].contiguous(), 1.0)
    assert torch.equal(want[0], first[0]) and torch.equal(want[1], first[1])
    _check(_replay(e), a, 0.0, want, path="replay")


def test_whole_waves_leave_the_loop_beside_waves_that_run_on():
    """3 agents, B = 5, C = 32: 64 pairs per workgroup and 16 per wave, pair b C + c - env 2 (past its episode's end: one counted
    step) owns pairs 64 ... 95, two whole waves of the second workgroup, which leave the K-loop after its first iteration while
    the workgroup's other waves run all K = 7 steps."""
    N, c, k = 3, 32, 7
    e = rt.env(N, B, k)
    a = rt.candidates(c, k, B, N)
    want = _check(e, a, 0.97)
    assert want[2].tolist() == [2, k, 1, k, k]
    _check(_replay(e), a, 0.97, want, path="replay")


def test_non_default_world_constants_reach_the_launch(golden):
    """dt, damping, contact force and margin, mass and the episode length of fixture hd_n9_constants, set on the World as a user
    sets them (they reach the launch through `Scenario.params`): both routes equal the reference, whose `env.rollout` runs under
    the same constants, and the returns are not those of the defaults."""
    g = golden("hd_n9_constants")
    N = 9
    e = rt.env(N, B, K)
    a = rt.candidates(C, K, B, N)
    default = e.rollout_returns(a, 0.97)[0].clone()
    w = e.world
    w.dt, w.damping = float(g["world_dt"]), float(g["world_damping"])
    w.contact_force, w.contact_margin = float(g["world_contact_force"]), float(g["world_contact_margin"])
    w.world_length = e.world_length = int(g["world_world_length"])
    for agent in w.agents:
        agent.initial_mass = float(g["world_mass"])
    assert int(w.world_length) == 7 != 100 and (w.dt, w.damping, w.contact_force, w.contact_margin) == (0.05, 0.4, 60.0, 0.004)
    w.step_count.copy_(rt.phases(B, K, int(w.world_length)))
    p = e.scenario.params(w)
    assert (p.mass, p.world_length) == (2.5, 7) and abs(p.dt - 0.05) < 1e-8 and abs(p.contact_force - 60.0) < 1e-5
    want = _check(e, a, 0.97)
    assert want[2].tolist() == [2, K, 1, K, 1]                       # phases 5, 1, 10, 0, 37 of an episode of 7 steps
    assert not torch.equal(want[0][:, 2], default[:, 2])            # one step from the same state: the constants are in it
    _check(_replay(e), a, 0.97, want, path="replay")


@pytest.mark.parametrize("route", ["fused", "replay"])
def test_non_contiguous_and_float64_candidates(route):
    """Candidates handed over as a permuted view of a [K, C, ...] tensor and as float64 give the bits of the contiguous fp32 call,
    and the caller's tensor is left as it was."""
    N = 9
    e = rt.env(N, B, K)
    if route == "replay":
        _replay(e)
    a = rt.candidates(C, K, B, N)
    want = _check(e, a, 0.97, path=route)
    kc = a.transpose(0, 1).contiguous()                              # [K, C, B, N, 2]
    view = kc.transpose(0, 1)
    assert not view.is_contiguous() and torch.equal(view, a)
    wide = a.double()
    for other in (view, wide):
        kept = other.clone()
        _check(e, other, 0.97, want, path=route)
        assert torch.equal(other, kept) and other.dtype == kept.dtype and other.stride() == kept.stride()
    assert torch.equal(kc, a.transpose(0, 1))


# ---- the fp32 product against the fp64 oracle: the one direct link ----
@pytest.mark.parametrize("N", rt.FUSED_N)
def test_fused_returns_against_the_fp64_oracle(N):
    """`rollout_returns` on the fused route against `rt.oracle_returns` (NumPy float64 on the env's own fp32 state and
    candidates), K = 3, gamma = 0.97, on the (candidate, env) pairs whose collision counts stay more than 1e-4 from flipping -
    at least 80 % of them.  Bound: rt.F32_ORACLE_BOUND x max(1, |R|), twice the largest error measured over the eight agent
    counts rounded up to one digit (profiles/returns_parity.md); the launch is deterministic, the factor covers another compiler
    build.  tests/test_returns_cpu.py holds every mutant of the recurrence to 100 x this bound."""
    k = 3
    e = rt.env(N, B, k)
    a = rt.candidates(C, k, B, N)
    assert e.returns_path() == "fused"
    shared, indiv, steps, margin = rt.oracle_returns(rt.oracle_state_of(e), a.double().cpu().numpy(), 0.97)
    ret, info = e.rollout_returns(a, 0.97)
    assert info["steps"].cpu().tolist() == steps.tolist() == [2, k, 1, k, k]
    ok = margin > rt.F32_MARGIN                                      # [C, B]
    assert ok.mean() >= 0.8, ok.mean()
    worst = 0.0
    for got, ref in ((ret, shared), (info["individual_return"], indiv)):
        rel = np.abs(got.double().cpu().numpy() - ref) / np.maximum(1.0, np.abs(ref))
        worst = max(worst, float(rel[ok].max()))
    print("N = %2d: largest |R32 - R64| / max(1, |R64|) = %.3g on %.3f of the pairs" % (N, worst, ok.mean()))
    assert worst <= rt.F32_ORACLE_BOUND, (N, worst)
