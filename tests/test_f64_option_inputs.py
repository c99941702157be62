"""CPU companion of tests/test_gpu_f64_options.py (oracle only, no GPU): the teeth of the fp64 free-running check of the
World-option kernel depend on WHICH branches its inputs take, so that is pinned here.

For every option branch an oracle blind to it must leave the trajectory (positions or individual rewards) by more than 1e-6
on a named input of the GPU tests; the oracle itself free-runs the reference's option fixtures exactly; rounding-level noise
stays two orders below the GPU tests' 1e-9; walls rounded to fp32 - the deviation only the fp64 check can see - land above it."""
import numpy as np
import pytest

from oracle import formation_oracle as O
from tests import option_cases as OC

MULTI_ENV = [n for n in OC.OPTION_FIXTURES if n not in OC.SINGLE_ENV and not n.endswith("_constants")]      # the seven with options


def _fixture_run(golden, name, **kw):
    c = OC.fixture_case(name, golden(name))
    r = OC.oracle_free_run(OC.fixture_state(c), np.asarray(c["g"]["acts"], dtype=np.float64), c["P"], c["opts"], c["comm"], **kw)
    return c, r


def _left_by(r, ref):
    """how far a run leaves a trajectory: positions and individual rewards"""
    return max(np.abs(r["pos"] - ref["pos"]).max(), np.abs(r["indiv"] - ref["indiv"]).max())


@pytest.mark.parametrize("name", OC.OPTION_FIXTURES)
def test_oracle_free_runs_on_the_option_fixtures(golden, name):
    """The fp64 oracle, free-running over the whole horizon (no re-seeding), stays on the reference: the 1e-9 of the GPU test is
    four orders above what the restatement itself differs by.  Measured maxima over the ten: pos 6.4e-14, vel 1.7e-13, indiv 4e-15."""
    c, r = _fixture_run(golden, name)
    g = c["g"]
    assert np.abs(r["pos"] - g["pos"]).max() <= 2e-13 and np.abs(r["vel"] - g["vel"]).max() <= 5e-13
    ok = g["cnt_margin"] > 1e-9
    assert ok.mean() >= 0.9
    assert np.abs(r["indiv"] - g["indiv"])[ok].max() <= 1e-13
    assert np.abs(r["shared"][..., None] - g["shared"])[ok].max() <= 1e-13 * max(1.0, np.abs(g["shared"]).max())
    for t in g["obs_steps"]:
        assert np.abs(r["obs"][t - 1] - g["obs_t%d" % t]).max() <= 5e-13


# branch -> (the fixture of the GPU test that takes it, how the oracle is blinded)
FIXTURE_BRANCHES = [
    ("wall force", "hd_n27_walls", dict(drop=("walls",))),
    ("corner rounding of a wall", "hd_n9_options", dict(blind=("corner",))),
    ("soft-wall pass-through of ghosts", "hd_n9_flags", dict(drop=("ghost",))),
    ("active speed clamp", "hd_n9_options", dict(drop=("max_speed",))),
    ("accel gain", "hd_n9_options", dict(drop=("accel",))),
    ("accel gain, per agent", "hd_n9_masses", dict(drop=("accel",))),
    ("mass ratio", "hd_n9_masses", dict(blind=("mass_ratio",))),
    ("immovable-partner rule", "hd_n6_immovable", dict(blind=("immovable_partner",))),
    ("non-colliding agents", "hd_n9_flags", dict(drop=("collide",))),
    ("per-pair penalty distance", "hd_n9_masses", dict(blind=("pair_distance",))),
]


@pytest.mark.parametrize("branch,name,how", FIXTURE_BRANCHES, ids=[b[0] for b in FIXTURE_BRANCHES])
def test_option_fixtures_take_the_branch(golden, branch, name, how):
    c, r = _fixture_run(golden, name, **how)
    assert _left_by(r, c["g"]) > 1e-6, "%s: an oracle blind to the %s stays on the reference" % (name, branch)


# every branch again on the seeded cases: env 0 of OC.seeded_case is arranged for them
SEEDED_BRANCHES = [
    ("wall force", dict(drop=("walls",))),
    ("corner rounding of a wall", dict(blind=("corner",))),
    ("soft-wall pass-through of ghosts", dict(drop=("ghost",))),
    ("active speed clamp", dict(drop=("max_speed",))),
    ("accel gain", dict(drop=("accel",))),
    ("mass ratio", dict(blind=("mass_ratio",))),
    ("immovable-partner rule", dict(blind=("immovable_partner",))),
    ("non-colliding agents", dict(drop=("collide",))),
    ("per-pair penalty distance", dict(blind=("pair_distance",))),
]


@pytest.fixture(scope="module")
def seeded():
    cache = {}

    def get(N, B):
        if (N, B) not in cache:
            c = OC.seeded_case(N, B)
            cache[(N, B)] = (c, OC.oracle_free_run(c["state"], c["acts"], c["P"], c["opts"]))
        return cache[(N, B)]
    return get


@pytest.mark.parametrize("N,B", OC.SEEDED_SHAPES)
def test_seeded_cases_show_contacts_and_wall_forces(seeded, N, B):
    c, r = seeded(N, B)
    assert r["cnt"].sum() > 0 and r["wall_hits"] > 0 and np.isfinite(r["pos"]).all()
    assert (r["cnt_margin"] > 1e-9).mean() >= 0.9
    o = c["opts"]
    assert 0.5 <= o["mass"].min() and o["mass"].max() <= 4 and 0.02 <= o["size"].min() and o["size"].max() <= 0.06
    assert (~o["movable"]).sum() == 1 and (~o["collide"]).sum() == 1 and o["ghost"].sum() == 1
    assert np.isnan(o["accel"]).any() and (~np.isnan(o["accel"])).any() and (~np.isnan(o["max_speed"])).any()
    hard = [w for w in o["walls"] if len(w) == 4 or w[4]]
    assert len(hard) == 2 and len(o["walls"]) == 3


@pytest.mark.parametrize("N,B", OC.SEEDED_SHAPES)
def test_seeded_cases_do_not_amplify_one_rounding_to_the_bound(seeded, N, B):
    """The GPU test holds the kernel to 1e-10 on these inputs over six steps: legitimate only where the inputs themselves carry
    rounding-level differences (the kernel's summation order) through six steps far below that.  One rounding of the initial
    positions moves every observation (positions and velocities) by at most 2e-12, 50 times below the bound."""
    c, r = seeded(N, B)
    for seed in (1, 2):
        st = dict(c["state"])
        st["pos"] = st["pos"] * (1 + 1e-16 * np.random.RandomState(seed).standard_normal(st["pos"].shape))
        r2 = OC.oracle_free_run(st, c["acts"], c["P"], c["opts"])
        assert np.abs(r2["obs"] - r["obs"]).max() <= 2e-12 and np.abs(r2["pos"] - r["pos"]).max() <= 2e-12


@pytest.mark.parametrize("N,B", OC.SEEDED_SHAPES)
@pytest.mark.parametrize("branch,how", SEEDED_BRANCHES, ids=[b[0] for b in SEEDED_BRANCHES])
def test_seeded_cases_take_the_branch(seeded, N, B, branch, how):
    c, r = seeded(N, B)
    blind = OC.oracle_free_run(c["state"], c["acts"][:2], c["P"], c["opts"], **how)
    ref = dict(pos=r["pos"][:2], indiv=r["indiv"][:2])
    assert _left_by(blind, ref) > 1e-6, "seeded_case(%d, %d): an oracle blind to the %s stays on the trajectory" % (N, B, branch)


def _perturbed(golden, name, scale, seed=0):
    c = OC.fixture_case(name, golden(name))
    st = OC.fixture_state(c)
    st["pos"] = st["pos"] * (1 + scale * np.random.RandomState(seed).standard_normal(st["pos"].shape))
    r = OC.oracle_free_run(st, np.asarray(c["g"]["acts"], dtype=np.float64), c["P"], c["opts"], c["comm"])
    return np.abs(r["pos"][-1] - c["g"]["pos"][-1]).max()


def test_rounding_level_noise_stays_far_below_the_bound(golden):
    """What summation order can cause: the initial positions multiplied by 1 + 1e-16 N(0,1) - noise of the size of one rounding -
    move the final positions of the multi-env option fixtures by at most 3.5e-12 (hd_n27_constants; hd_n9_options ... 1e-13),
    1e-14 noise by at most 2.3e-10.  The GPU test's 1e-9 is more than two orders above the first."""
    small = {n: _perturbed(golden, n, 1e-16) for n in MULTI_ENV + ["hd_n9_constants", "hd_n27_constants"]}
    large = {n: _perturbed(golden, n, 1e-14) for n in MULTI_ENV + ["hd_n9_constants", "hd_n27_constants"]}
    print(small, large)
    assert max(small.values()) <= 1e-11, small
    assert max(large.values()) <= 1e-9, large


@pytest.mark.parametrize("name", ["hd_n9_options", "hd_n27_masses", "hd_n9_flags", "hd_n27_walls"])
def test_walls_rounded_to_fp32_leave_the_bound(golden, name):
    """The deviation only the fp64 check sees: the wall constants alone rounded to fp32 (0.9f, 0.6f, 0.1f ...), everything else
    in double, move the trajectory by 4.6e-8 (hd_n9_options), 1.4e-7 (hd_n27_masses), 8.5e-8 (hd_n9_flags), 8.8e-6 (hd_n27_walls) -
    above the 1e-9 of the fp64 test by more than a factor of 40, and three of the four below the fp32 tests' 1e-5."""
    c = OC.fixture_case(name, golden(name))
    f32 = lambda x: float(np.float32(x))
    walls = [(w[0], f32(w[1]), (f32(w[2][0]), f32(w[2][1])), f32(w[3])) + tuple(w[4:]) for w in c["opts"]["walls"]]
    r = OC.oracle_free_run(OC.fixture_state(c), np.asarray(c["g"]["acts"], dtype=np.float64), c["P"], dict(c["opts"], walls=walls),
                           c["comm"])
    moved = np.abs(r["pos"] - c["g"]["pos"]).max()
    print(name, moved)
    assert moved > 4e-8
    if name != "hd_n27_walls":
        assert moved < 1e-5
