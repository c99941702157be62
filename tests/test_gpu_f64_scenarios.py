"""The run-time-count kernel of the four landmark scenarios - fg::scn_kernel (csrc/fg_scn_kernel.hpp): contact forces among agents
and obstacles, per-agent tables and flags, walls, the obstacle velocity re-arm and floor, the formation terms, collision counts,
the ring / clipped / plain neighbour blocks, both observation writers, the K-loop - in the fp64 parity build
(csrc/formation_hip_f64.hip, fg64_rollout_scenario: the SAME source with real = double), FREE-RUNNING over the reference's 14
landmark fixtures from their initial state against the reference's float64 arrays, and against the fp64 oracle at every
lane-group width and workgroup size.  The fp32 product is held to these fixtures one teacher-forced step at a time at 1e-5; an
agent size or obs_range passed through `float` moves them by 1e-8 ... 4e-6 and only shows here
(tests/test_f64_scenario_inputs.py, which also pins the branches these inputs take).

Bounds: fixtures 1e-9 abs (shared reward: relative to max(1, |shared|)), as the other fp64 tests; oracle cases 1e-10 over six
steps.  The measured maxima are in profiles/f64_scenarios.md."""
import numpy as np
import pytest

from tests import scenario_cases as SC

pytestmark = pytest.mark.gpu
FIXTURE_TOL = 1e-9
ORACLE_TOL = 1e-10


def _env(c, stage, state=None):
    from tests import f64_parity
    N = c["state"]["pos"].shape[1]
    return f64_parity.Scn64(c["kind"], c["state"] if state is None else state, c["P"],
                            options=f64_parity.kernel_options(N, c["P"], **c["opts"]), stage=stage)


def _no_sentinel(out, what):
    from tests import f64_parity
    for k in ("obs", "reward", "indiv"):
        assert np.isfinite(out[k]).all() and not (out[k] == f64_parity.SENTINEL).any(), "%s: %s not written everywhere" % (what, k)
    assert not (out["done"] == 7).any(), "%s: done not written everywhere" % what
    if "near_ag" in out:
        assert (out["near_ag"] >= 0).all(), "%s: near_ag not written everywhere" % what


def _same_bits(a, b, what):
    for k in a:
        if a[k] is None:
            assert b[k] is None
            continue
        np.testing.assert_array_equal(a[k], b[k], err_msg="%s: %s" % (what, k))


def fixture_errors(c, out, state):
    """max abs deviation of a free run (outputs [T, ...], end state) from the fixture, by quantity"""
    ref = c["ref"]
    err = dict(pos=np.abs(state["pos"] - ref["pos"][-1]).max(), vel=np.abs(state["vel"] - ref["vel"][-1]).max(),
               obs=np.abs(out["obs"] - ref["obs"]).max(), indiv=np.abs(out["indiv"] - ref["indiv"]).max())
    if ref["shared"] is not None:
        err["shared"] = (np.abs(out["reward"] - ref["shared"]) / np.maximum(1.0, np.abs(ref["shared"]))).max()
    if c["kind"] == "obstacle":
        err["opos"] = np.abs(state["obst_pos"] - ref["opos"][-1]).max()
        err["ovel"] = np.abs(state["obst_vel"] - ref["ovel"][-1]).max()
    return err


def _check_near_ag(c, near, pos):
    """basic: near_ag [T,B,L] = the agent nearest to each landmark, recomputed from the FIXTURE's positions [T,B,N,2]; compared
    wherever the two smallest distances differ by more than 1e-9"""
    lm = c["state"]["landmarks"]
    D = np.sqrt(((pos[:, :, :, None, :] - lm[None, :, None, :, :]) ** 2).sum(-1))          # [T,B,a,l]
    two = np.sort(D, axis=2)[:, :, :2]
    clear = (two[:, :, 1] - two[:, :, 0]) > 1e-9
    assert clear.mean() > 0.9
    np.testing.assert_array_equal(near[clear], D.argmin(2)[clear])


@pytest.mark.parametrize("name", [f[0] for f in SC.FIXTURES])
def test_f64_scenario_kernel_free_runs_on_the_reference_trajectory(golden, name):
    """The whole horizon from the fixture's initial state with its own actions, table, flags and walls: as T single-step launches
    and as ONE launch with K = T, each with both observation writers (bit-identical outputs), every step's positions, velocities,
    obstacle state, observations, rewards and done flags against the fixture."""
    c = SC.fixture_case(name, golden(name))
    ref, acts = c["ref"], c["acts"]
    T = acts.shape[0]
    runs = {}
    for stage in (0, 1):
        env = _env(c, stage)
        steps = {k: [] for k in ("pos", "vel", "opos", "ovel")}
        outs = []
        for t in range(T):                                   # T launches with K = 1: the state after every step is read back
            outs.append(env.step(acts[t]))
            s = env.state()
            steps["pos"].append(s["pos"]); steps["vel"].append(s["vel"]); steps["opos"].append(s["obst_pos"]); steps["ovel"].append(s["obst_vel"])
        single = {k: np.stack([o[k] for o in outs]) for k in outs[0]}
        end_single = env.state()
        roll_env = _env(c, stage)
        roll = roll_env.rollout(acts)                         # ONE launch through the K-loop
        end_roll = roll_env.state()
        what = "%s stage %d" % (name, stage)
        _no_sentinel(single, what + " single steps")
        _no_sentinel(roll, what + " K-loop")
        _same_bits(single, roll, what + ": the K-loop against single steps")
        _same_bits(end_single, end_roll, what + ": end state of the K-loop against single steps")
        assert (end_roll["step"] == T).all()
        # every step, env and agent against the fixture
        assert np.abs(np.stack(steps["pos"]) - ref["pos"]).max() <= FIXTURE_TOL, what
        assert np.abs(np.stack(steps["vel"]) - ref["vel"]).max() <= FIXTURE_TOL, what
        if c["kind"] == "obstacle":
            assert np.abs(np.stack(steps["opos"]) - ref["opos"]).max() <= FIXTURE_TOL, what
            assert np.abs(np.stack(steps["ovel"]) - ref["ovel"]).max() <= FIXTURE_TOL, what
        err = fixture_errors(c, roll, end_roll)
        print(what, {k: "%.2e" % v for k, v in err.items()})
        for k, v in err.items():
            assert v <= FIXTURE_TOL, "%s: %s error %.3g over %d free-running steps (bound %.0e)" % (what, k, v, T, FIXTURE_TOL)
        if ref["done"] is not None:
            np.testing.assert_array_equal(roll["done"], ref["done"].astype(np.uint8), err_msg=what)
        else:                                                 # driven through core.py's World API: no episode ends inside it
            assert T < c["P"].world_length and not roll["done"].any()
        if c["kind"] == "basic":
            _check_near_ag(c, roll["near_ag"], ref["pos"])
        runs[stage] = (roll, end_roll)
    _same_bits(runs[0][0], runs[1][0], name + ": staged against unstaged outputs")
    _same_bits(runs[0][1], runs[1][1], name + ": staged against unstaged end state")


def oracle_errors(c, r, out, state, obs_every=1):
    """max abs deviation of a K-step launch from the oracle's free run `r`; individual and shared rewards over the (step, env)
    entries with no pair within 1e-9 of a collision threshold.  Returns (errors, share of entries compared)."""
    ok = r["margin"] > 1e-9
    err = dict(pos=np.abs(state["pos"] - r["pos"][-1]).max(), vel=np.abs(state["vel"] - r["vel"][-1]).max(),
               obs=np.abs(out["obs"] - r["obs"][obs_every - 1::obs_every]).max(),
               indiv=np.abs(out["indiv"] - r["indiv"])[ok].max(),
               shared=(np.abs(out["reward"] - r["shared"][..., None]) / np.maximum(1.0, np.abs(r["shared"][..., None])))[ok].max())
    if c["kind"] == "obstacle":
        err["opos"] = np.abs(state["obst_pos"] - r["opos"][-1]).max()
        err["ovel"] = np.abs(state["obst_vel"] - r["ovel"][-1]).max()
    return err, ok.mean()


def _against_the_oracle(c):
    """A case through the K-loop: stage 0 with obs_every 1 and 2, stage 1 (where the image fits; -2 where it does not) bit for bit
    the same; everything against the oracle's free run.  Returns the errors of the stage-0 launch."""
    r = SC.oracle_free_run(c["kind"], c["state"], c["acts"], c["P"], c["opts"])
    K, B, N = c["acts"].shape[:3]
    env = _env(c, 0)
    out = env.rollout(c["acts"])
    end = env.state()
    what = c["name"]
    _no_sentinel(out, what)
    err, share = oracle_errors(c, r, out, end)
    print(what, {k: "%.2e" % v for k, v in err.items()}, "compared %.2f" % share)
    assert share >= 0.9
    for k, v in err.items():
        assert v <= ORACLE_TOL, "%s: %s error %.3g after %d free-running steps (bound %.0e)" % (what, k, v, K, ORACLE_TOL)
    np.testing.assert_array_equal(out["done"], r["done"].astype(np.uint8), err_msg=what)
    assert (end["step"] == c["state"]["step"] + K).all()
    env2 = _env(c, 0)
    out2 = env2.rollout(c["acts"], obs_every=2)               # every second observation, everything else as before
    assert out2["obs"].shape[0] == K // 2
    np.testing.assert_array_equal(out2["obs"], out["obs"][1::2], err_msg=what + " obs_every 2")
    _same_bits({k: v for k, v in out2.items() if k != "obs"}, {k: v for k, v in out.items() if k != "obs"}, what + " obs_every 2")
    _same_bits(env2.state(), end, what + " obs_every 2")
    fits = SC.lds_bytes(c["kind"], N, c["P"], True) <= SC.FG64_LDS_LIMIT
    env3 = _env(c, 1)
    rc, out3 = env3.launch(c["acts"], obs_every=2 if N % 2 else 1)
    if fits:
        assert rc == 0, "%s: the staged launch returned %d" % (what, rc)
        ref3 = out2 if N % 2 else out
        _same_bits(out3, ref3, what + ": staged against unstaged outputs")
        _same_bits(env3.state(), end, what + ": staged against unstaged end state")
    else:
        assert rc == -2, "%s: a staged image of %d bytes must be refused, got %d" % (what, SC.lds_bytes(c["kind"], N, c["P"], True), rc)
        s3 = env3.state()
        assert np.array_equal(s3["pos"], c["state"]["pos"]) and np.array_equal(s3["step"], c["state"]["step"]), what + ": a refused launch touched the state"
    return err


@pytest.mark.parametrize("i", range(len(SC.SEEDED)), ids=[SC.seeded_id(s) for s in SC.SEEDED])
def test_f64_scenario_kernel_against_the_oracle_at_other_counts(i):
    """Six free-running steps in ONE launch at every lane-group width (4 ... 64 lanes per env, every kind) and every
    whole-workgroup size (128 ... 1024 threads), ragged last workgroups, crowded starts, a per-agent table with every flag beyond
    64 entities; staged and unstaged writers, obs_every 1 and 2."""
    _against_the_oracle(SC.seeded_case(i))


@pytest.mark.parametrize("N,B", SC.FLOOR_SHAPES)
def test_f64_scenario_kernel_at_the_obstacle_floor(N, B):
    """formation_hd_obs_env.py:84-89 where no fixture goes: one obstacle crosses obstacle_floor inside the launch, one lies below
    it with velocity 0 and is pushed by the agent under it (re-armed where that lifts it above the floor), one keeps falling."""
    c = SC.floor_case(N, B)
    r = SC.oracle_free_run(c["kind"], c["state"], c["acts"], c["P"], c["opts"])
    s = SC.floor_states(c, r)
    assert s["falling"][:, 2].all() and s["crossing"][:, 0].all() and s["moved"][:, 1].all()
    _against_the_oracle(c)
    # ... and as single steps: the obstacle state after every step
    env = _env(c, 0)
    for t in range(c["acts"].shape[0]):
        env.step(c["acts"][t])
        st = env.state()
        assert np.abs(st["obst_pos"] - r["opos"][t]).max() <= ORACLE_TOL and np.abs(st["obst_vel"] - r["ovel"][t]).max() <= ORACLE_TOL, t


def test_bad_arguments_are_refused():
    from tests import f64_parity
    c = SC.seeded_case(4)
    env = _env(c, 0)
    env.stage = 2
    assert env.launch(c["acts"])[0] == -1
    env.stage = 0
    assert env.launch(c["acts"], obs_every=0)[0] == -1
    assert env.launch(c["acts"], do_physics=0)[0] == -1        # K > 1 without physics
    env.scenario.kind = 9
    assert env.launch(c["acts"][:1])[0] == -1
    assert np.array_equal(env.state()["pos"], c["state"]["pos"]), "a refused launch touched the state"
    assert f64_parity.SCN_KINDS["obstacle"] == 4
