"""CPU companion of tests/test_gpu_f64_scenarios.py (oracle only, no GPU): the teeth of the fp64 free-running check of the landmark
scenario kernel depend on WHICH branches its inputs take and on the oracle itself staying on the reference, so both are pinned
here.

The oracle free-runs the 14 landmark fixtures over their whole horizons four orders below the GPU test's 1e-9 with no pair near a
collision threshold; for every branch an oracle blind to it leaves the trajectory by more than 1e-6 on a named input of the GPU
tests; an agent size or obs_range rounded to fp32 - the deviation only the fp64 check can see - lands above 1e-9; the seeded and
floor cases keep at least 90 % of their (env, step) entries away from a threshold and do not amplify one rounding to the bound."""
import numpy as np
import pytest

from tests import scenario_cases as SC


def _fixture_run(golden, name, **kw):
    c = SC.fixture_case(name, golden(name))
    return c, SC.oracle_free_run(c["kind"], c["state"], c["acts"], c["P"], c["opts"], **kw)


def _left_by(r, ref, keys=("pos", "obs", "indiv")):
    """how far a run leaves a trajectory"""
    return max(np.abs(r[k] - ref[k]).max() for k in keys)


@pytest.mark.parametrize("name", [f[0] for f in SC.FIXTURES])
def test_oracle_free_runs_on_the_landmark_fixtures(golden, name):
    """No re-seeding over the whole horizon.  Measured maxima over the 14: positions 3.2e-14, velocities and observations 1.2e-13
    (range_n7_crowd), individual rewards 2e-15, shared rewards 1.8e-14 (partial_n9_crowd); done flags identical; no pair closer than
    2.8e-4 (obst_n5_masses) to its collision threshold, so no entry of any fixture needs excusing."""
    c, r = _fixture_run(golden, name)
    ref = c["ref"]
    assert np.abs(r["pos"] - ref["pos"]).max() <= 2e-13
    assert np.abs(r["vel"] - ref["vel"]).max() <= 5e-13 and np.abs(r["obs"] - ref["obs"]).max() <= 5e-13
    assert np.abs(r["indiv"] - ref["indiv"]).max() <= 1e-13 * max(1.0, np.abs(ref["indiv"]).max())
    if ref["shared"] is not None:
        assert np.abs(r["shared"][..., None] - ref["shared"]).max() <= 1e-13 * max(1.0, np.abs(ref["shared"]).max())
    if ref["done"] is not None:
        assert np.array_equal(r["done"], ref["done"])
    if c["kind"] == "obstacle":
        assert np.abs(r["opos"] - ref["opos"]).max() <= 2e-13 and np.abs(r["ovel"] - ref["ovel"]).max() <= 5e-13
    assert r["margin"].min() > 2e-4, "a pair within %g of its collision threshold" % r["margin"].min()


def test_episodes_end_inside_four_fixtures(golden):
    for name in ("basic_n3", "partial_n5", "range_n4", "obst_n4"):
        done = golden(name)["done"]
        assert done[-1].all() and not done[0].any()


# branch -> (the fixture of the GPU test that takes it, how the oracle is blinded, the quantities that must leave)
FIXTURE_BRANCHES = [
    ("agent-obstacle contact force", "obst_n8", dict(obstacle_size=0.0), ("pos",)),
    ("obstacle velocity re-arm", "obst_n4", dict(obstacle_floor=np.inf), ("obs",)),
    ("range clipping", "range_n4", dict(obs_range=np.inf), ("obs",)),
    ("ring neighbours", "partial_n5", dict(blind=("ring",)), ("obs",)),
    ("self-collision of basic", "basic_n3", dict(blind=("self",)), ("indiv",)),
    ("obstacle penalty of 2", "obst_n5_masses", dict(penalty=1.0), ("indiv",)),
    ("mass ratio", "partial_n6_masses", dict(drop=("mass",)), ("pos",)),
    ("mass ratio", "obst_n5_masses", dict(drop=("mass",)), ("pos",)),
    ("immovable partner", "partial_n6_immovable", dict(drop=("movable",)), ("pos",)),
    ("immovable partner", "obst_n5_immovable", dict(drop=("movable",)), ("pos",)),
    ("non-colliding agent", "obst_n5_flags", dict(drop=("collide",)), ("pos", "indiv")),
    ("non-colliding agent", "basic_n4_flags", dict(drop=("collide",)), ("pos", "indiv")),
    ("ghost at a soft wall", "obst_n5_flags", dict(drop=("ghost",)), ("pos",)),
    ("per-agent speed clamp", "obst_n5_masses", dict(drop=("max_speed",)), ("pos",)),
    ("per-pair contact distance", "partial_n6_masses", dict(drop=("size",)), ("pos", "indiv")),
]


@pytest.mark.parametrize("branch,name,how,keys", FIXTURE_BRANCHES, ids=["%s-%s" % (b[0], b[1]) for b in FIXTURE_BRANCHES])
def test_fixtures_take_the_branch(golden, branch, name, how, keys):
    c, r = _fixture_run(golden, name, **how)
    for k in keys:
        assert np.abs(r[k] - c["ref"][k]).max() > 1e-6, "%s: an oracle blind to the %s stays on the reference's %s" % (name, branch, k)


def test_range_n4_clips_many_of_its_differences(golden):
    """more than a quarter of the relative-position components of range_n4 lie beyond obs_range (36 % of them sit on +-0.7)"""
    c = SC.fixture_case("range_n4", golden("range_n4"))
    N, L = c["state"]["pos"].shape[1], c["P"].num_landmarks
    rel = c["ref"]["obs"][..., 2 + 2 * L:2 + 2 * L + 2 * (N - 1)]
    assert 0.25 < (np.abs(rel) == c["P"].obs_range).mean() < 0.5


@pytest.mark.parametrize("name,over,key", [("partial_n9_crowd", "agent_size", "pos"), ("range_n7_crowd", "agent_size", "pos"),
                                           ("range_n4", "obs_range", "obs")])
def test_constants_rounded_to_fp32_leave_the_bound(golden, name, over, key):
    """The deviation only the fp64 check can see: the agent size 0.04 (it sets the contact distance) or obs_range 0.7 fed as their
    fp32 neighbours, everything else in double.  Measured: 2.8e-7 (partial_n9_crowd) and 4.2e-6 (range_n7_crowd) on the positions,
    1.2e-8 on the clipped observations of range_n4 - above the 1e-9 of the fp64 test, below the fp32 tests' 1e-5."""
    c = SC.fixture_case(name, golden(name))
    exact = getattr(c["P"], over)
    r = SC.oracle_free_run(c["kind"], c["state"], c["acts"], c["P"], c["opts"], **{over: float(np.float32(exact))})
    moved = np.abs(r[key] - c["ref"][key]).max()
    print(name, over, moved)
    assert 1e-9 < moved < 1e-5


# ---------------------------------------------------------------------------
# the seeded cases and the floor cases of the GPU tests
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    cache = {}

    def get(key):
        if key not in cache:
            c = SC.seeded_case(key) if isinstance(key, int) else SC.floor_case(*key)
            cache[key] = (c, SC.oracle_free_run(c["kind"], c["state"], c["acts"], c["P"], c["opts"]))
        return cache[key]
    return get


def test_seeded_cases_cover_every_geometry():
    """every kind at every lane-group width; every whole-workgroup size; ragged last workgroups; images that fit and that do not"""
    geo = {}
    for kind, N, B, crowd, table in SC.SEEDED:
        G, T, E, D = SC.geometry(kind, N, SC.params(kind))
        geo.setdefault(G, []).append((kind, B % E != 0 or E == 1, SC.lds_bytes(kind, N, SC.params(kind), True) <= SC.FG64_LDS_LIMIT, table))
    for G in (4, 8, 16, 32, 64):
        assert {k for k, _, _, _ in geo[G]} == {"basic", "partial", "range", "obstacle"}, G
        assert all(ragged for _, ragged, _, _ in geo[G]), G
    assert all(G in geo for G in (128, 256, 512, 1024))
    fits = [f for v in geo.values() for _, _, f, _ in v]
    assert any(fits) and not all(fits)
    assert any(f for G in (128,) for _, _, f, _ in geo[G]), "no whole-workgroup case with a staged image"
    assert any(t for G in (128, 256, 512, 1024) for _, _, _, t in geo[G]), "no per-agent table beyond 64 entities"


@pytest.mark.parametrize("i", range(len(SC.SEEDED)), ids=[SC.seeded_id(c) for c in SC.SEEDED])
def test_seeded_cases_keep_the_excused_share_small_and_do_not_amplify_rounding(runs, i):
    """The GPU test holds the kernel to 1e-10 over six steps on these inputs and compares individual rewards where no pair is within
    1e-9 of a threshold: at least 90 % of the (env, step) entries; and ONE rounding of the initial positions moves no observation by
    more than 5e-12 (measured: 2.2e-12 at 1000 agents, 1e-14 at a handful), 20 times below the bound."""
    c, r = runs(i)
    assert np.isfinite(r["obs"]).all() and (r["margin"] > 1e-9).mean() >= 0.9
    contact = (r["indiv"] != r["indiv"].max(-1, keepdims=True)).any() if c["kind"] != "basic" else (r["indiv"].max(-1) - r["indiv"].min(-1) > 0.5).any()
    assert contact or c["state"]["pos"].shape[1] == 1, "no collision penalty anywhere: the start is not crowded"
    st = dict(c["state"])
    st["pos"] = st["pos"] * (1 + 1e-16 * np.random.RandomState(1).standard_normal(st["pos"].shape))
    r2 = SC.oracle_free_run(c["kind"], st, c["acts"], c["P"], c["opts"])
    assert np.abs(r2["obs"] - r["obs"]).max() <= 5e-12 and np.abs(r2["pos"] - r["pos"]).max() <= 5e-12


TABLE_CASE = [i for i, c in enumerate(SC.SEEDED) if c[4]][0]
TABLE_BRANCHES = [("mass ratio", "mass"), ("immovable partner", "movable"), ("non-colliding agent", "collide"),
                  ("ghost at a soft wall", "ghost"), ("per-agent speed clamp", "max_speed"), ("wall force", "walls")]


@pytest.mark.parametrize("branch,drop", TABLE_BRANCHES, ids=[b[0] for b in TABLE_BRANCHES])
def test_table_case_takes_the_branch(runs, branch, drop):
    """the per-agent table beyond 64 entities: env 0 is arranged so that every flag decides something within two steps"""
    c, r = runs(TABLE_CASE)
    assert c["state"]["pos"].shape[1] + c["P"].num_obstacles > 64
    blind = SC.oracle_free_run(c["kind"], c["state"], c["acts"][:2], c["P"], c["opts"], drop=(drop,))
    assert np.abs(blind["pos"][:, 0] - r["pos"][:2, 0]).max() > 1e-6, "an oracle blind to the %s stays on the trajectory" % branch


@pytest.mark.parametrize("N,B", SC.FLOOR_SHAPES)
def test_floor_cases_show_the_three_obstacle_states(runs, N, B):
    """From the oracle's own run: obstacle 2 keeps falling, obstacle 0 crosses the floor inside the launch, obstacle 1 - stopped
    below the floor - is moved by the agent under it (and where that lifts it above the floor its velocity is re-armed); an oracle
    without the floor (or with everything below it) leaves the trajectory, as do one without the agent-obstacle contact and one
    with the other scenarios' penalty of 1."""
    c, r = runs((N, B))
    s = SC.floor_states(c, r)
    assert s["falling"][:, 2].all() and s["crossing"][:, 0].all() and s["moved"][:, 1].all()
    assert (r["ovel"][-1][:, 0] == 0).all() and (r["ovel"][:, :, 2] == c["P"].obstacle_vel).all()
    assert (r["margin"] > 1e-9).mean() >= 0.9 and np.isfinite(r["obs"]).all()
    for branch, how, key in (("floor stop", dict(obstacle_floor=-np.inf), "obs"), ("velocity re-arm", dict(obstacle_floor=np.inf), "obs"),
                             ("agent-obstacle contact force", dict(obstacle_size=0.0), "pos"), ("obstacle penalty of 2", dict(penalty=1.0), "indiv")):
        blind = SC.oracle_free_run(c["kind"], c["state"], c["acts"], c["P"], c["opts"], **how)
        assert np.abs(blind[key] - r[key]).max() > 1e-6, "floor case: an oracle blind to the %s stays on the trajectory" % branch


def test_floor_cases_re_arm_a_stopped_obstacle_somewhere(runs):
    """over the two shapes a pushed, stopped obstacle ends up above the floor (velocity re-armed from zero) in some envs and stays
    below it (velocity stays zero) in others"""
    s = [SC.floor_states(*runs(k))["rearmed"][:, 1] for k in SC.FLOOR_SHAPES]
    assert np.concatenate(s).any() and not np.concatenate(s).all()
