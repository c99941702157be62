"""Every device implementation of the built-in controller on inputs that take every branch of `ezpolicy`.

The case sets of tests/policy_testlib.py (formed at chosen levels and sub-groups, the 0.01 threshold from both sides, natural
against reference alignment, active clips, late own marks and the fallback, exact ties; tests/test_policy_cases_cpu.py pins on
the CPU that they reach those branches and that a model carrying a wrong rule leaves the bound on them) go through
  (a) `bfs_actions` on oracle-built fp32 observations          policy_bfs_kernel, levels at run time
  (b) `scenario.policy_actions` from the simulator state       policy_state_kernel
  (c) `env.rollout_policy(2, per)`, first step's actions       the pipelined closed-loop kernels (bfs_policy_env, levels at
                                                               compile time) at 64 envs, the case set tiled
  (d) the same at 32768 envs of 3 and 4 agents                 hd_lane_kernel (bfs_policy_lane: the controller on registers)
  (e) 36 agents, 6 per layer                                   chained controller and step launches
and are held to the fp64 oracle at the controller's existing bound, 1e-5 x max(1, the env's largest action component), with NO
excused row: the cases keep every comparison 1e-4 (mostly 1e-3) from a tie, and the ties of the `ties` class are exact in both
precisions.  (b) equals (a) bit for bit, and so do (c), (d), (e)."""
import numpy as np
import pytest
import torch

from tests import policy_testlib as T

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().double().cpu().numpy()


def _hold_to_oracle(got, per, L, what):
    """got [B, N, 2] on `T.stacked(per, L)`; prints the worst err / bound of every class"""
    want = T.reference(per, L)
    ratio = np.abs(got - want).max(-1) / T.bound(want)[:, None]               # [B, N]
    print("%-18s per %d L %d N %3d: worst err / bound %s" % (
        what, per, L, per ** L, "  ".join("%s %.3f" % (c, ratio[s].max()) for c, s in T.stacked(per, L)[2].items())))
    for c, s in T.stacked(per, L)[2].items():
        assert (ratio[s] <= 1.0).all(), "%s, class %s: %d row(s) off the fp64 oracle, worst %.3g x the bound, and no row is excused" % (
            what, c, int((ratio[s] > 1.0).sum()), ratio[s].max())


@pytest.fixture(scope="module")
def standalone():
    """(a): the stand-alone launch's actions per hierarchy, computed once and shared (a device tensor [B, N, 2])"""
    cache = {}

    def get(per, L):
        if (per, L) not in cache:
            from formation_gym.policy_bfs import bfs_actions
            obs = torch.as_tensor(T.stacked(per, L)[1].astype(np.float32)).cuda()
            cache[(per, L)] = bfs_actions(obs, per)
        return cache[(per, L)]
    return get


def _env(per, L, idx):
    """formation_hd_env holding envs `idx` of the hierarchy's case set: no auto-reset, step counters at zero"""
    import formation_gym
    case = T.stacked(per, L)[0]
    env = formation_gym.make_env("formation_hd_env", False, per ** L, num_envs=len(idx), device="cuda:0")
    env.world.set_state(case["pos"][idx], np.zeros_like(case["pos"][idx]))
    env.scenario.set_formation(env.world, case["shape"][idx], case["ivel"][idx])
    env.world.step_count.zero_()
    env.auto_reset = False
    return env


@pytest.mark.parametrize("per,L", T.HIERARCHIES, ids=["%dx%d" % h for h in T.HIERARCHIES])
def test_standalone_controller_launches(standalone, per, L):
    act = standalone(per, L)
    assert act.dtype == torch.float32 and torch.isfinite(act).all()
    _hold_to_oracle(_np(act), per, L, "(a) policy_bfs")
    env = _env(per, L, np.arange(act.shape[0]))
    assert torch.equal(env.scenario.policy_actions(env.world, per), act)        # (b): from the state, the same bits


def _closed_loop(standalone, per, L, batch, what):
    ref = standalone(per, L)
    B = ref.shape[0]
    got = torch.empty_like(ref)
    for start in range(0, B, batch):
        idx = (start + np.arange(batch)) % B                                     # the case set, tiled to fill the batch
        env = _env(per, L, idx)
        act = env.rollout_policy(2, per)[3]["actions"][0]
        at = torch.as_tensor(idx).cuda()
        assert torch.equal(act, ref[at]), "%s differs from the stand-alone launch" % what
        got[at] = act
    _hold_to_oracle(_np(got), per, L, what)


@pytest.mark.parametrize("per,L", T.CLOSED_LOOP, ids=["%dx%d" % h for h in T.CLOSED_LOOP])
def test_pipelined_closed_loop_kernels(standalone, per, L):
    _closed_loop(standalone, per, L, T.CLOSED_LOOP_BATCH, "(c) rollout_policy")


@pytest.mark.parametrize("per,L", [(3, 1), (2, 2)], ids=["3x1", "2x2"])
def test_one_env_per_lane_kernels(standalone, per, L):
    _closed_loop(standalone, per, L, T.LANE_BATCH, "(d) hd_lane_kernel")


@pytest.mark.parametrize("per,L", T.CHAINED, ids=["%dx%d" % h for h in T.CHAINED])
def test_chained_closed_loop(standalone, per, L):
    _closed_loop(standalone, per, L, T.CLOSED_LOOP_BATCH, "(e) chained")
