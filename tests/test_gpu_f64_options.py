"""The World-option half of the fused step kernel - step_kernel<..., OPTS = true>: action_force with accel, clamp_speed,
wall_forces (corner rounding, soft walls, ghosts), agent_props_of, contact_force_het (mass ratio, per-pair contact distance,
the immovable-partner rule), collision_count_het, the communication block of the flat writer, the properties re-fetched per
step by the 1024-thread instantiation - in the fp64 parity build (csrc/formation_hip_f64.hip, fg64_step_hd_opts), FREE-RUNNING
over the reference's option fixtures from their initial state, against the reference's float64 arrays.  The fp32 product is
held to these fixtures one teacher-forced step at a time at 1e-5; a wall constant passed through `float` moves them by 5e-8 ...
9e-6 and only shows here (tests/test_f64_option_inputs.py, which also pins the branches these inputs take).

Bound: 1e-9 abs, as tests/test_gpu_f64_parity.py.  Measured maxima on an MI355X (profiles/r02_parity_errors.md):
positions <= 7.6e-15 on the eight option fixtures (hd_n27_masses) and 4.7e-13 on hd_n27_constants (the stiffest: contact margin
2e-3 at force 150, dt 0.2), velocities <= 1.2e-12, individual rewards <= 1.3e-14, shared (relative) <= 2.9e-15, observations
<= 1.1e-12; no done, index or excused collision-count mismatch.  Seeded oracle cases at 5 ... 600 agents after six steps:
positions <= 3.8e-15, velocities / observations <= 1.7e-14, individual rewards <= 8.9e-16 (bound 1e-10)."""
import numpy as np
import pytest

from tests import option_cases as OC
from tests import parity_errors as PE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case(golden):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = OC.fixture_case(name, golden(name))
        return cache[name]
    return get


@pytest.mark.parametrize("name", OC.OPTION_FIXTURES)
def test_f64_option_kernel_free_runs_on_the_reference_trajectory(case, name):
    """All recorded steps, one launch per step: positions, velocities, individual and shared rewards, done flags, the index
    assignments away from ties and every recorded observation (hd_n5_comm: with the fixture's `c` as comm_state; hd_n6_scripted:
    FG_AGENT_SCRIPTED and the reference's u_scripted)."""
    c = case(name)
    r = PE.free_running_f64(c["g"], P=c["P"], options=c["opts"], comm=c["comm"])
    print(name, r["err"], r["idx_bad"])
    tol = 1e-9
    for k, v in r["err"].items():
        assert v <= tol, "%s: %s error %.3g over %d free-running steps (bound %.0e); positions per step %s" % (
            name, k, v, r["steps"], tol, " ".join("%.1e" % x for x in r["per_step_pos"]))
    assert r["idx_bad"]["done"] == 0
    assert r["idx_bad"]["near_lm"] == 0 and r["idx_bad"]["near_ag"] == 0      # bit-exact away from exact ties
    assert r["idx_bad"]["cnt_excused"] <= 0.1 * r["steps"] * r["envs"]        # env-steps with a collision count on its threshold
    assert np.isfinite(r["per_step_pos"]).all()


@pytest.mark.parametrize("name", ["hd_n9_options", "hd_n27_masses"])
def test_one_launch_of_the_k_loop_equals_single_step_launches(case, name):
    """The whole horizon through the kernel's own K-loop (K = T, as the product runs option rollouts) = T launches with K = 1:
    the same fp64 values, bit for bit - so the K-loop stays on the fixture as well."""
    from tests import f64_parity
    c = case(name)
    g = c["g"]
    T, B, N = g["acts"].shape[:3]
    acts = np.asarray(g["acts"], dtype=np.float64)
    mk = lambda: f64_parity.Env64(g["pos0"], g["vel0"], g["ideal_shape"], g["ideal_vel"], params=f64_parity.params_of(c["P"]),
                                  options=f64_parity.kernel_options(N, c["P"], **c["opts"]))
    a, b = mk(), mk()
    ro = a.rollout(acts)
    for t in range(T):
        b.step(acts[t])
        np.testing.assert_array_equal(ro["obs"][t], b.obs.cpu().numpy())
        np.testing.assert_array_equal(ro["reward"][t], b.reward.cpu().numpy())
        np.testing.assert_array_equal(ro["indiv"][t], b.indiv.cpu().numpy())
        np.testing.assert_array_equal(ro["done"][t], b.done.cpu().numpy())
    np.testing.assert_array_equal(a.pos(), b.pos())
    np.testing.assert_array_equal(a.vel(), b.vel())
    np.testing.assert_array_equal(a.step_count.cpu().numpy(), np.full(B, T))
    for k in ("near_lm", "near_ag", "hd_idx"):
        np.testing.assert_array_equal(getattr(a, k).cpu().numpy(), getattr(b, k).cpu().numpy())
    assert np.abs(a.pos() - g["pos"][-1]).max() <= 1e-9 and np.isfinite(ro["obs"]).all()


@pytest.mark.parametrize("N,B", OC.SEEDED_SHAPES)
def test_f64_option_kernel_against_the_oracle_at_other_agent_counts(N, B):
    """Every lane-group width, the whole-workgroup reduction and the 1024-thread instantiation (600 agents: the properties
    re-fetched inside the step loop) with a random per-agent table - masses 0.5 ... 4, sizes 0.02 ... 0.06, accel / max_speed on
    about half the agents, an immovable, a non-colliding and a ghost agent - among two hard walls and a soft one: 6 free-running
    steps against the fp64 oracle at 1e-10.  tests/test_f64_option_inputs.py shows on the CPU that each case has contacts and wall
    forces, takes every option branch, and carries one rounding of its initial state through the six steps below 2e-12."""
    from oracle import formation_oracle as O
    from tests import f64_parity
    c = OC.seeded_case(N, B)
    st, opts = c["state"], c["opts"]
    env = f64_parity.Env64(st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], params=f64_parity.params_of(c["P"]),
                           options=f64_parity.kernel_options(N, c["P"], **opts))
    worst = dict(pos=0.0, vel=0.0, indiv=0.0, obs=0.0)
    for t in range(OC.SEEDED_STEPS):
        st, out = O.step_hd(st, c["acts"][t], c["P"], **opts)
        env.step(c["acts"][t])
        ok = out["cnt_margin"] > 1e-9
        got = dict(pos=env.pos(), vel=env.vel(), indiv=env.indiv.cpu().numpy()[ok], obs=env.obs.cpu().numpy())
        want = dict(pos=st["pos"], vel=st["vel"], indiv=out["indiv"][ok], obs=out["obs"])
        for k in worst:
            worst[k] = max(worst[k], PE._mx(got[k], want[k]))
        print(N, B, t, worst)
        for k in worst:
            np.testing.assert_allclose(got[k], want[k], rtol=0, atol=1e-10, err_msg="%s at step %d" % (k, t))


def test_option_entry_refuses_a_workgroup_that_does_not_fit_the_lds():
    """1024 agents with the option tables in 8-byte values need 172 608 bytes of LDS, more than a gfx950 workgroup has: the
    entry says so (-2) instead of launching; 600 agents (101 376 bytes, above the 64 KiB default) run."""
    import torch
    from tests import f64_parity
    N = 1024
    z = np.zeros((1, N, 2))
    env = f64_parity.Env64(z, z, z, np.zeros((1, 2)), options=f64_parity.kernel_options(N, None))
    act = torch.zeros((1, N, 2), dtype=torch.float64, device="cuda")
    p = lambda t: t.data_ptr()
    rc = f64_parity.load().fg64_step_hd_opts(env.params, env.options, 1, N, 1, p(env.px), p(env.py), p(env.vx), p(env.vy), p(act),
                                             p(env.shape), p(env.ivel), p(env.step_count), p(env.obs), p(env.reward), p(env.indiv),
                                             p(env.done), p(env.near_lm), p(env.near_ag), p(env.hd_idx), None)
    assert rc == -2
    assert (env.step_count.cpu().numpy() == 0).all()
