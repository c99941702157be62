"""GPU parity tests: the HIP path (through the C ABI and the Python env shell)
against the golden fixtures captured from the reference and against the CPU
oracle.  Run with `pytest -m gpu` on an MI355X.

Tolerances (BASELINE.json north_star): 1e-5 abs in fp32 for positions, velocities,
observations and individual rewards - every such bound in this file is ATOL = 1e-5, none is
looser; the maxima actually measured are 3e-7 (positions), 2.6e-6 (velocities = position
error / dt), 1.1e-6 (observations), 2.8e-7 (individual rewards), committed per fixture in
profiles/r02_parity_errors.md.  They are checked PER STEP with the state re-seeded from the
reference (teacher forcing) and free-running over a short horizon - stiff contact springs make
longer fp32 trajectories diverge chaotically; the full-length free-running
check is the fp64 build of the same kernel source, tests/test_gpu_f64_parity.py (<= 7e-12).
The ONE relative bound: the shared reward is a sum of N individual rewards (|r| up to ~270 at
N=243, where one fp32 ulp is 3e-5 > 1e-5 abs), so it is checked at 2e-6 relative + 1e-5 abs
(measured: 1.8e-7 relative) (H2).
done masks are bit-exact; landmark-index assignments are bit-exact except
where the reference's own top-2 gap is < 1e-6 (a genuine fp32 near-tie, H5).
"""
import numpy as np
import pytest
import torch

from oracle import formation_oracle as O

pytestmark = pytest.mark.gpu

ATOL = 1e-5
HD_CASES = ["hd_n3", "hd_n9", "hd_n27", "hd_n81", "hd_n9_crowd", "hd_n27_crowd",
            "hd_n81_crowd", "hd_n243", "hd_n4", "hd_n10", "hd_n5", "hd_n6_crowd", "hd_n16_crowd", "hd_n50", "hd_n100_crowd"]


def _make(N, B, scenario="formation_hd_env"):
    import formation_gym
    return formation_gym.make_env(scenario, False, N, num_envs=B, device="cuda:0")


def _load(env, pos, vel, shape, ivel, step):
    env.world.set_state(pos, vel)
    env.scenario.set_formation(env.world, shape, ivel)
    env.world.step_count.copy_(torch.as_tensor(np.asarray(step, dtype=np.int32)))


def _np(t):
    return t.detach().double().cpu().numpy()


def _check_indices(got, want, gap, what):
    bad = got != want
    if bad.any():
        assert (gap[bad] < 1e-6).all(), "%s mismatch away from a near-tie" % what


@pytest.mark.parametrize("name", HD_CASES)
def test_step_teacher_forced(golden, name):
    g = golden(name)
    T, B, N = g["acts"].shape[:3]
    env = _make(N, B)
    env.enable_assignments(True)
    prev_pos, prev_vel = g["pos0"], g["vel0"]
    for t in range(T):
        _load(env, prev_pos, prev_vel, g["ideal_shape"], g["ideal_vel"], np.full(B, t))
        act = torch.as_tensor(g["acts"][t]).cuda()
        obs, rew, done, info = env.step(act)
        pos, vel = env.world.get_state()
        np.testing.assert_allclose(_np(pos), g["pos"][t], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(vel), g["vel"][t], rtol=0, atol=ATOL)
        # rewards are functions of the post-step state; compare on the GPU's own state
        # against the oracle evaluated on that same fp32 state ...
        r = O.reward_hd(_np(pos), _np(vel), g["ideal_shape"].astype(np.float32).astype(np.float64),
                        g["ideal_vel"].astype(np.float32).astype(np.float64), O.HdParams())
        margin_ok = r["cnt_margin"] > 1e-6
        ind = _np(info["individual_reward"])
        np.testing.assert_allclose(ind[margin_ok], r["indiv"][margin_ok], rtol=0, atol=ATOL)
        # ... and against the reference's numbers where no collision count sits on the edge
        ref_ok = g["cnt_margin"][t] > 1e-5
        np.testing.assert_allclose(ind[ref_ok], g["indiv"][t][ref_ok], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(rew)[ref_ok, :, 0], g["shared"][t][ref_ok], rtol=2e-6, atol=ATOL)
        assert rew.shape == (B, N, 1) and done.shape == (B, N) and done.dtype == torch.bool
        np.testing.assert_array_equal(done.cpu().numpy(), g["done"][t])
        _check_indices(env._out["near_lm"].cpu().numpy(), r["near_lm"], r["gap_lm"], "near_lm")
        _check_indices(env._out["near_ag"].cpu().numpy(), r["near_ag"], r["gap_ag"], "near_ag")
        hd = env._out["hd_idx"].cpu().numpy()
        tie = r["hd_gap"].min(1) < 1e-6
        np.testing.assert_array_equal(hd[~tie], r["hd_idx"][~tie])
        if (t + 1) in g["obs_steps"]:
            want = O.observation_hd(_np(pos), _np(vel), g["ideal_shape"], g["ideal_vel"])
            np.testing.assert_allclose(_np(obs), want, rtol=0, atol=2e-7)       # same fp32 state
            np.testing.assert_allclose(_np(obs), g["obs_t%d" % (t + 1)], rtol=0, atol=ATOL)
        prev_pos, prev_vel = g["pos"][t], g["vel"][t]


@pytest.mark.parametrize("name", ["hd_n3", "hd_n9", "hd_n27", "hd_n81", "hd_n27_crowd", "hd_n4"])
def test_free_running_short_horizon(golden, name):
    g = golden(name)
    T, B, N = g["acts"].shape[:3]
    env = _make(N, B)
    _load(env, g["pos0"], g["vel0"], g["ideal_shape"], g["ideal_vel"], np.zeros(B))
    # fp32 free-running error per fixture and step: profiles/r02_parity_errors.md (hd_n81: 6.4e-6 after 10 steps,
    # hd_n27_crowd: 1.1e-6 after 5, 1e-5 after 10).  The horizon is what stays inside 1e-5; beyond it contacts amplify
    # fp32 rounding chaotically (H1) and the fp64 build of the kernel carries the check (test_gpu_f64_parity.py)
    H = 5 if "crowd" in name else 10
    for t in range(min(H, T)):
        env.step(torch.as_tensor(g["acts"][t]).cuda())
        pos, vel = env.world.get_state()
        np.testing.assert_allclose(_np(pos), g["pos"][t], rtol=0, atol=ATOL)
    assert (env.world.step_count.cpu().numpy() == min(H, T)).all()


def test_done_flips_at_world_length(golden):
    g = golden("hd_n3_done")
    T, B, N = g["acts"].shape[:3]
    env = _make(N, B)
    _load(env, g["pos0"], g["vel0"], g["ideal_shape"], g["ideal_vel"], np.zeros(B))
    for t in range(T):
        _, _, done, _ = env.step(torch.as_tensor(g["acts"][t]).cuda())
        np.testing.assert_array_equal(done.cpu().numpy(), g["done"][t])     # bit-exact
    assert env.world_length == 100


@pytest.mark.parametrize("N,B", [(9, 7), (27, 5), (81, 3), (10, 6), (100, 2)])
def test_split_stages_equal_fused(N, B):
    """fg_physics_step + fg_observe_hd == fg_step_hd, bit for bit."""
    rs = np.random.RandomState(N)
    st = O.reset_hd(rs.randint(0, 10000, B), N)
    st["pos"] *= 0.3
    act = torch.as_tensor(rs.uniform(-1, 1, (B, N, 2)).astype(np.float32)).cuda()
    fused = _make(N, B); _load(fused, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], st["step"])
    split = _make(N, B); _load(split, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], st["step"])
    obs, rew, done, info = fused.step(act)
    split.world.action_u.copy_(act)
    split.world.step()
    out = dict(obs=torch.empty_like(obs), reward=torch.empty((B, N), device="cuda"),
               indiv=torch.empty((B, N), device="cuda"))
    split.scenario.observe_batch(split.world, out)
    for a, b in zip(fused.world.get_state(), split.world.get_state()):
        assert torch.equal(a, b)
    assert torch.equal(obs, out["obs"])
    assert torch.equal(rew[..., 0], out["reward"])
    assert torch.equal(info["individual_reward"], out["indiv"])
    # per-agent plugin callbacks return that agent's slice
    ag = fused.agents[N // 2]
    assert torch.equal(fused._get_obs(ag), obs[:, ag.i])
    assert torch.equal(fused._get_reward(ag), info["individual_reward"][:, ag.i])


@pytest.mark.parametrize("N,B,K", [(9, 10, 6), (27, 6, 5), (81, 2, 4), (243, 2, 3)])
def test_rollout_equals_single_steps(N, B, K):
    rs = np.random.RandomState(100 + N)
    st = O.reset_hd(rs.randint(0, 10000, B), N)
    st["pos"] *= 0.4
    acts = torch.as_tensor(rs.uniform(-1, 1, (K, B, N, 2)).astype(np.float32)).cuda()
    a = _make(N, B); _load(a, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], st["step"])
    b = _make(N, B); _load(b, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], st["step"])
    out = dict(obs=torch.empty((K, B, N, 6 * N), device="cuda"), reward=torch.empty((K, B, N), device="cuda"),
               indiv=torch.empty((K, B, N), device="cuda"),
               done=torch.zeros((K, B, N), dtype=torch.uint8, device="cuda"))
    b.scenario.rollout_batch(b.world, acts, out)
    for k in range(K):
        obs, rew, done, info = a.step(acts[k])
        assert torch.equal(obs, out["obs"][k])
        assert torch.equal(rew[..., 0], out["reward"][k])
        assert torch.equal(info["individual_reward"], out["indiv"][k])
        assert torch.equal(done, out["done"][k].bool())
    for x, y in zip(a.world.get_state(), b.world.get_state()):
        assert torch.equal(x, y)
    assert torch.equal(a.world.step_count, b.world.step_count)
    # obs_every: only every 2nd observation is written
    c = _make(N, B); _load(c, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], st["step"])
    out2 = dict(obs=torch.zeros((K // 2, B, N, 6 * N), device="cuda"), reward=torch.empty((K, B, N), device="cuda"))
    c.scenario.rollout_batch(c.world, acts, out2, obs_every=2)
    for s in range(K // 2):
        assert torch.equal(out2["obs"][s], out["obs"][2 * s + 1])
    assert torch.equal(out2["reward"], out["reward"])


@pytest.mark.parametrize("N,B", [(27, 4096), (9, 4096), (81, 256), (243, 96), (3, 1000)])
def test_full_size_against_oracle_and_invariants(N, B):
    """BASELINE-size batches: fp64 oracle on every env + size-independent properties."""
    seeds = 1 + 1000 * np.arange(B)
    st = O.reset_hd(seeds, N)
    rs = np.random.RandomState(0)
    act = rs.uniform(-1, 1, (B, N, 2)).astype(np.float32)
    env = _make(N, B)
    _load(env, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], st["step"])
    obs, rew, done, info = env.step(torch.as_tensor(act).cuda())
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    st32 = dict(st, pos=f32(st["pos"]), ideal_shape=f32(st["ideal_shape"]), ideal_vel=f32(st["ideal_vel"]))
    chunk = 64 if N >= 81 else 1024
    pos, vel = (_np(x) for x in env.world.get_state())
    ind = _np(info["individual_reward"]); shared = _np(rew)[..., 0]; o = _np(obs)
    for s in range(0, B, chunk):
        sl = slice(s, min(B, s + chunk))
        sub = {k: v[sl] for k, v in st32.items()}
        new, out = O.step_hd(sub, act[sl].astype(np.float64))
        np.testing.assert_allclose(pos[sl], new["pos"], rtol=0, atol=ATOL)
        np.testing.assert_allclose(vel[sl], new["vel"], rtol=0, atol=ATOL)
        ok = out["cnt_margin"] > 1e-5
        np.testing.assert_allclose(ind[sl][ok], out["indiv"][ok], rtol=0, atol=ATOL)
        np.testing.assert_allclose(shared[sl][ok], out["reward"][ok][..., 0], rtol=2e-6, atol=ATOL)
        np.testing.assert_allclose(o[sl], out["obs"], rtol=0, atol=ATOL)
    # invariants
    assert not done.any()
    np.testing.assert_allclose(ind.sum(1), shared[:, 0], rtol=2e-6, atol=1e-4)   # shared = sum of individuals
    assert (shared == shared[:, :1]).all()                                      # broadcast to every agent
    assert (o[:, :, 2 * N:4 * N - 2] == 0).all()                                # comm block
    assert (o[:, :, 4 * N - 2:6 * N - 2] == f32(st["ideal_shape"]).reshape(B, 1, 2 * N)).all()
    assert (o[:, :, 6 * N - 2:] == f32(st["ideal_vel"])[:, None]).all()
    assert (o[:, :, 0:2] == vel).all()
    # antisymmetry of the relative-position block: obs_i[j] = -obs_j[i]
    i, j = 0, N - 1
    np.testing.assert_array_equal(o[:, i, 2 + 2 * (j - 1):4 + 2 * (j - 1)], -o[:, j, 2 + 2 * i:4 + 2 * i])
    # batch independence: the same envs in a smaller batch give bit-identical results
    nb = min(B, 37)
    env2 = _make(N, nb)
    _load(env2, st["pos"][:nb], st["vel"][:nb], st["ideal_shape"][:nb], st["ideal_vel"][:nb], st["step"][:nb])
    obs2, rew2, _, info2 = env2.step(torch.as_tensor(act[:nb]).cuda())
    assert torch.equal(obs2, obs[:nb]) and torch.equal(rew2, rew[:nb])
    assert torch.equal(info2["individual_reward"], info["individual_reward"][:nb])


def test_reference_style_api_single_env(golden):
    """num_envs == 1: list-in / list-out exactly like the reference."""
    g = golden("hd_n9")
    import formation_gym
    env = formation_gym.make_env("formation_hd_env", benchmark=False, num_agents=9)
    assert env.num_envs == 1 and env.num_agents == 9 and env.world_length == 100
    assert env.observation_space[0].shape == (54,) and env.share_observation_space[0].shape == (486,)
    assert env.action_space[0].shape == (2,) and env.action_space[0].sample().dtype == np.float32
    env.seed(int(g["seed"]))
    obs_n = env.reset()
    assert isinstance(obs_n, list) and len(obs_n) == 9 and obs_n[0].shape == (54,) and obs_n[0].dtype == np.float64
    np.testing.assert_allclose(np.array(obs_n), g["obs0"][0], rtol=0, atol=ATOL)   # same MT19937 stream
    for t in range(5):
        act_n = [g["acts"][t, 0, i].astype(np.float64).copy() for i in range(9)]
        keep = [a.copy() for a in act_n]
        obs_n, rew_n, done_n, info_n = env.step(act_n)
        np.testing.assert_allclose(np.array(act_n), 5.0 * np.array(keep))          # scaled in place
        np.testing.assert_allclose(np.array([x['individual_reward'] for x in info_n]), g["indiv"][t, 0], atol=ATOL)
        assert rew_n[0] == rew_n[8] and isinstance(rew_n[0], list)
        np.testing.assert_allclose(rew_n[0][0], g["shared"][t, 0, 0], rtol=2e-6, atol=ATOL)
        assert done_n == [False] * 9
    with pytest.raises(TypeError):
        env.step([[0.0, 0.0]] * 9)                                                # lists rejected like the reference


def test_seeded_reset_matches_reference_stream(golden):
    g = golden("reset")
    import formation_gym
    for seed, N in g["cases"]:
        env = formation_gym.make_env("formation_hd_env", False, int(N), num_envs=2, device="cuda:0")
        env.seed(int(seed))
        obs = env.reset()
        key = "s%d_n%d" % (seed, N)
        np.testing.assert_allclose(_np(obs[0]), g[key + "_obs"], rtol=0, atol=1e-6)
        # env 1 uses seed + 1000 (worker convention); (1, 9)+1000 = (1001, 9) is also a fixture
        if (seed + 1000, N) in [tuple(c) for c in g["cases"]]:
            np.testing.assert_allclose(_np(obs[1]), g["s%d_n%d_obs" % (seed + 1000, N)], rtol=0, atol=1e-6)


def test_basic_formation_env(golden):
    g = golden("basic_n3")
    env = _make(3, 1, "basic_formation_env")
    assert env.world_length == 50 and env.observation_space[0].shape == (18,)
    env.world.set_state(g["pos0"], g["vel0"])
    env.world.landmark_pos.copy_(torch.as_tensor(g["landmarks"], dtype=torch.float32))
    env.world.step_count.zero_()
    out = {"obs": env._out["obs"], "reward": env._out["reward"]}
    env.scenario.observe_batch(env.world, out)
    np.testing.assert_allclose(_np(out["obs"]), g["obs0"], rtol=0, atol=ATOL)
    prev_pos, prev_vel = g["pos0"], g["vel0"]
    for t in range(g["acts"].shape[0]):
        env.world.set_state(prev_pos, prev_vel)
        obs, rew, done, info = env.step(torch.as_tensor(g["acts"][t]).cuda())
        pos, vel = env.world.get_state()
        np.testing.assert_allclose(_np(pos), g["pos"][t], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(obs), g["obs"][t], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(info["individual_reward"]), g["indiv"][t], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(rew)[..., 0], g["shared"][t], rtol=2e-6, atol=ATOL)
        np.testing.assert_array_equal(done.cpu().numpy(), g["done"][t])
        prev_pos, prev_vel = g["pos"][t], g["vel"][t]


def test_auto_reset_vec_env_semantics():
    """Device-side reset: reset obs with pre-reset reward/done, fresh state in range."""
    from formation_gym.vec_env import FormationVecEnv
    N, B = 9, 64
    env = _make(N, B)
    env.seed(3)
    venv = FormationVecEnv(env, reset_mode="device")
    venv.reset()
    env.world.step_count.fill_(98)
    act = torch.zeros((B, N, 2), device="cuda")
    obs, rew, done, info = venv.step(act)
    assert not done.any()
    shape_before = env.scenario.ideal_shape.clone()
    obs, rew, done, info = venv.step(act)
    assert done.all()                                         # pre-reset done
    assert (env.world.step_count == 0).all()
    pos, vel = env.world.get_state()
    assert (vel == 0).all() and (pos.abs() <= 1).all() and pos.std() > 0.4
    assert not torch.equal(shape_before, env.scenario.ideal_shape)
    np.testing.assert_allclose(_np(env.scenario.ideal_shape.mean(1)), 0, atol=1e-6)
    want = O.observation_hd(_np(pos), _np(vel), _np(env.scenario.ideal_shape), _np(env.scenario.ideal_vel))
    np.testing.assert_allclose(_np(obs), want, rtol=0, atol=1e-6)    # obs is the RESET observation
    assert torch.isfinite(rew).all()
    # envs differ from each other and from the next reset
    assert pos[0].ne(pos[1]).any()
    env.world.step_count.fill_(99)
    venv.step(act)
    pos2, _ = env.world.get_state()
    assert pos2.ne(pos).any()


def test_host_reset_vec_env_parity_mode():
    from formation_gym.vec_env import FormationVecEnv
    N, B = 3, 4
    env = _make(N, B)
    env.seed(11)
    venv = FormationVecEnv(env, reset_mode="host")
    venv.reset()
    env.world.step_count[1] = 99
    obs, rew, done, info = venv.step(torch.zeros((B, N, 2), device="cuda"))
    assert done[1].all() and not done[0].any()
    assert int(env.world.step_count[1]) == 0 and int(env.world.step_count[0]) == 1
    # env 1 continued its own MT19937 stream: second draw block of RandomState(11 + 1000)
    rs = np.random.RandomState(11 + 1000); rs.uniform(-1, 1, (2 * N + 1, 2))
    want = rs.uniform(-1, 1, (N, 2))
    pos, _ = env.world.get_state()
    np.testing.assert_allclose(_np(pos[1]), want, atol=1e-6)


def test_nan_on_coincident_agents_like_reference():
    """core.py:312: two agents at the same point -> 0/0 -> NaN state."""
    N, B = 3, 2
    env = _make(N, B)
    pos = np.array([[[0.1, 0.1], [0.1, 0.1], [0.5, 0.5]], [[0.0, 0.0], [0.3, 0.3], [0.6, 0.6]]])
    _load(env, pos, np.zeros((B, N, 2)), np.zeros((B, N, 2)), np.zeros((B, 2)), np.zeros(B))
    env.step(torch.zeros((B, N, 2), device="cuda"))
    p, _ = env.world.get_state()
    assert torch.isnan(p[0, 0]).all() and torch.isnan(p[0, 1]).all() and torch.isfinite(p[0, 2]).all()
    assert torch.isfinite(p[1]).all()


def test_bfs_policy_closed_loop_on_device():
    """The built-in hierarchical controller, batched on the GPU, reduces the formation error."""
    import formation_gym
    N, B = 9, 32
    env = _make(N, B)
    env.seed(5)
    obs = env.reset()
    first = None
    for t in range(60):
        act = formation_gym.get_action_BFS(formation_gym.ezpolicy, obs, 3).float().contiguous()
        obs, rew, done, info = env.step(act)
        if first is None:
            first = rew[:, 0, 0].clone()
    assert (rew[:, 0, 0] > first).float().mean() > 0.9


SCN_GPU = [("formation_hd_partial_env", "partial", "partial_n5"), ("formation_hd_partial_env", "partial", "partial_n9_crowd"),
           ("formation_hd_partial_env", "partial", "partial_n3"),
           ("formation_hd_partial_range_env", "range", "range_n4"), ("formation_hd_partial_range_env", "range", "range_n7_crowd"),
           ("formation_hd_obs_env", "obstacle", "obst_n4"), ("formation_hd_obs_env", "obstacle", "obst_n8")]


@pytest.mark.parametrize("scenario,kind,name", SCN_GPU)
def test_remaining_scenarios_teacher_forced(golden, scenario, kind, name):
    """formation_hd_partial_env / _partial_range_env / _obs_env through fg_step_scenario,
    re-seeded from the reference every step."""
    g = golden(name)
    P = O.ScnParams(kind)
    T, B, N = g["acts"].shape[:3]
    L = P.num_landmarks
    env = _make(N, B, scenario)
    assert env.world_length == P.world_length and env.observation_space[0].shape == (int(g["obs_dim"]),)

    def load(pos, vel, lm, lmvel, step):
        env.world.set_state(pos, vel)
        env.world.landmark_pos.copy_(torch.as_tensor(lm[:, :L], dtype=torch.float32))
        if P.num_obstacles:
            env.world.obstacle_pos.copy_(torch.as_tensor(lm[:, L:], dtype=torch.float32))
            env.world.obstacle_vel.copy_(torch.as_tensor(lmvel[:, L:], dtype=torch.float32))
        env.world.step_count.fill_(step)

    load(g["pos0"], g["vel0"], g["lm0"], g["lmvel0"], 0)
    out = {"obs": env._out["obs"], "reward": env._out["reward"]}
    env.scenario.observe_batch(env.world, out)
    np.testing.assert_allclose(_np(out["obs"]), g["obs0"], rtol=0, atol=ATOL)
    for t in range(T):
        if t:
            load(g["pos"][t - 1], g["vel"][t - 1], g["lm"][t - 1], g["lmvel"][t - 1], t)
        obs, rew, done, info = env.step(torch.as_tensor(g["acts"][t]).cuda())
        pos, vel = env.world.get_state()
        np.testing.assert_allclose(_np(pos), g["pos"][t], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(vel), g["vel"][t], rtol=0, atol=ATOL)
        if P.num_obstacles:
            np.testing.assert_allclose(_np(env.world.obstacle_pos), g["lm"][t][:, L:], rtol=0, atol=ATOL)
            np.testing.assert_allclose(_np(env.world.obstacle_vel), g["lmvel"][t][:, L:], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(obs), g["obs"][t], rtol=0, atol=ATOL)
        # collision counts are integers: excuse only pairs sitting on the threshold
        want = g["indiv"][t]
        bad = np.abs(_np(info["individual_reward"]) - want) > ATOL
        if bad.any():
            new, _ = O.step_scn(kind, dict(pos=g["pos"][t - 1] if t else g["pos0"], vel=g["vel"][t - 1] if t else g["vel0"],
                                           landmarks=(g["lm"][t - 1] if t else g["lm0"])[:, :L],
                                           obst_pos=(g["lm"][t - 1] if t else g["lm0"])[:, L:],
                                           obst_vel=(g["lmvel"][t - 1] if t else g["lmvel0"])[:, L:],
                                           step=np.full(B, t)), g["acts"][t].astype(np.float64), P)
            PD = np.sqrt(((new["pos"][:, :, None] - new["pos"][:, None]) ** 2).sum(-1)) + 10 * np.eye(N)
            assert (np.abs(PD - P.collide_thresh).min() < 1e-5), "individual reward mismatch away from a threshold"
        else:
            np.testing.assert_allclose(_np(rew)[..., 0], g["shared"][t], rtol=2e-6, atol=ATOL)
        np.testing.assert_array_equal(done.cpu().numpy(), g["done"][t])


@pytest.mark.parametrize("scenario,kind,name", [("formation_hd_obs_env", "obstacle", "obst_n5_masses"),
                                                ("formation_hd_partial_env", "partial", "partial_n6_masses")])
def test_landmark_scenarios_with_per_agent_tables(golden, scenario, kind, name):
    """Agents of different mass / size / max_speed in the landmark scenarios (FgParams.agent_props through fg_step_scenario:
    force ratio m_b / m_a core.py:314-317, contact and penalty distance size_a + size_b, per-agent speed clamp) among the
    obstacles of formation_hd_obs_env (:36-42), teacher-forced against the reference; K-step launch == single steps."""
    g = golden(name)
    P = O.ScnParams(kind)
    T, B, N = g["acts"].shape[:3]
    L = P.num_landmarks

    def build():
        env = _make(N, B, scenario)
        for a, m, s_, ms in zip(env.world.agents, g["agent_mass"], g["agent_size"], g["agent_max_speed"]):
            a.initial_mass = float(m); a.size = float(s_); a.max_speed = None if np.isnan(ms) else float(ms)
        return env

    def load(env, pos, vel, lm, lmvel, step):
        env.world.set_state(pos, vel)
        env.world.landmark_pos.copy_(torch.as_tensor(lm[:, :L], dtype=torch.float32))
        if P.num_obstacles:
            env.world.obstacle_pos.copy_(torch.as_tensor(lm[:, L:], dtype=torch.float32))
            env.world.obstacle_vel.copy_(torch.as_tensor(lmvel[:, L:], dtype=torch.float32))
        env.world.step_count.fill_(step)
    env = build()
    penalties = 0
    for t in range(T):
        src = (lambda k: g[k + "0"]) if t == 0 else (lambda k: g[k][t - 1])
        load(env, src("pos"), src("vel"), src("lm"), src("lmvel"), t)
        obs, rew, done, info = env.step(torch.as_tensor(g["acts"][t]).cuda())
        pos, vel = env.world.get_state()
        np.testing.assert_allclose(_np(pos), g["pos"][t], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(vel), g["vel"][t], rtol=0, atol=ATOL)
        if P.num_obstacles:
            np.testing.assert_allclose(_np(env.world.obstacle_pos), g["lm"][t][:, L:], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(obs), g["obs"][t], rtol=0, atol=ATOL)
        bad = np.abs(_np(info["individual_reward"]) - g["indiv"][t]) > ATOL
        if bad.any():                                        # integers: excuse only a pair sitting on its threshold
            sz = g["agent_size"]
            PD = np.sqrt(((g["pos"][t][:, :, None] - g["pos"][t][:, None]) ** 2).sum(-1)) + 10 * np.eye(N)
            assert np.abs(PD - (sz[:, None] + sz[None, :])).min() < 1e-5, "individual reward mismatch away from a threshold"
        penalties += int((g["indiv"][t] < -P.penalty + 0.5).sum())
    assert penalties > 0
    a, b = build(), build()
    for e in (a, b):
        load(e, g["pos0"], g["vel0"], g["lm0"], g["lmvel0"], 0)
    acts = torch.as_tensor(g["acts"][:8]).cuda().contiguous()
    o_seq, r_seq, d_seq, i_seq = b.rollout(acts)
    for t in range(8):
        o, r, d, i = a.step(acts[t])
        assert torch.equal(o, o_seq[t]) and torch.equal(r, r_seq[t]) and torch.equal(i["individual_reward"], i_seq["individual_reward"][t])


def test_remaining_scenarios_seeded_reset(golden):
    import formation_gym
    for scenario, name in [("formation_hd_partial_env", "partial_n5"), ("formation_hd_partial_range_env", "range_n4"),
                           ("formation_hd_obs_env", "obst_n4")]:
        g = golden(name)
        B, N = g["pos0"].shape[:2]
        env = formation_gym.make_env(scenario, False, N, num_envs=B, device="cuda:0")
        env.seed(int(g["seed"]))
        obs = env.reset()
        np.testing.assert_allclose(_np(obs), g["obs0"], rtol=0, atol=1e-6)     # same MT19937 streams
        # reference-style single env
        env1 = formation_gym.make_env(scenario, False, N)
        env1.seed(int(g["seed"]))
        o = env1.reset()
        assert isinstance(o, list) and len(o) == N
        np.testing.assert_allclose(np.array(o), g["obs0"][0], rtol=0, atol=1e-6)


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return str(sk.getsockname()[1])


def _run(cmd, env_extra=None, timeout=300):
    """Run a Python command from the repo root; on a timeout the WHOLE process group is killed (a launcher's rank
    processes would otherwise keep the pipes open and block this test for good)."""
    import os
    import signal
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **(env_extra or {}))
    proc = subprocess.Popen([sys.executable] + cmd, cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                            text=True, start_new_session=True)
    try:
        stdout, stderr = proc.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(proc.pid, signal.SIGKILL)
        stdout, stderr = proc.communicate()
        raise AssertionError("timed out after %d s: %s\n%s" % (timeout, " ".join(cmd), (stdout[-1500:] + stderr[-1500:])))
    assert proc.returncode == 0, stdout[-2000:] + stderr[-2000:]
    return stdout


def test_bench_json_contract_single_and_two_ranks():
    """bench.py prints ONE JSON line with the contract keys; the 2-rank path (barrier, MAX over
    ranks, sharded seeds, GLOBAL-batch configs) is exercised with two gloo ranks sharing this GPU."""
    import json
    line = [l for l in _run(["bench.py", "--steps", "30", "--warmup", "5", "--envs", "512", "--agents", "9", "--full",
                             "--no-cpu-baseline", "--global-div", "64"]).splitlines() if l.startswith("{")]
    assert len(line) == 1
    d = json.loads(line[0])
    # one GPU: the scaling efficiency of the GLOBAL-batch configs is 1.0 by construction (same-run denominator)
    assert [g["scaling_efficiency_vs_n1"] for g in d["global_configs"]] == [1.0, 1.0]
    assert all(g["n1_same_run"] and g["n1_env_steps_per_s"] == g["env_steps_per_s"] for g in d["global_configs"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "timing"):
        assert k in d
    assert d["n_gpus"] == 1 and d["steps"] == 30 and d["dtype"] == "f32" and d["roofline"]["bound"] == "hbm"
    assert d["state_finite"] and d["value"] > 0 and "workload" in d["config"]
    # roofline.traffic is measured on this box by two rocprofv3 --pmc child runs (or says why it could not be)
    r = d["roofline"]
    if str(r.get("traffic_source", "")).startswith("live"):
        assert 0.5 < r["traffic"] / r["algorithmic_bytes_per_launch"] < 1.5, r
    else:
        assert "traffic_live_error" in r, r
    # ONE clock: value, ms_per_step and roofline.achieved all come from ONE HIP-event series of exactly --steps steps
    t = d["timing"]
    assert t["timed_steps"] == 30 and t["blocks"] == 1 and t["block_ms_min"] == t["block_ms_median"] == t["block_ms_max"]
    assert abs(t["timed_ms_total"] - t["block_ms_median"]) < 1e-3
    assert abs(d["ms_per_step"] * 30 - t["block_ms_median"]) < 1e-3 * t["block_ms_median"] + 1e-5
    assert abs(d["value"] - 512 * 30 / (t["block_ms_median"] * 1e-3)) < 1e-3 * d["value"]
    alg = d["roofline"]["algorithmic_bytes_per_launch"] / d["config"]["steps_per_launch"] * 30
    assert abs(d["roofline"]["achieved"] - alg / (t["block_ms_median"] * 1e-3) / 1e9) < 1e-3 * d["roofline"]["achieved"] + 0.1
    out = _run(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", _free_port(), "bench.py", "--gpus", "2", "--steps", "20", "--warmup", "5", "--envs", "256",
                "--agents", "9", "--backend", "gloo", "--full", "--no-cpu-baseline", "--global-div", "64", "--min-timed-ms", "5"])
    line = [l for l in out.splitlines() if l.startswith("{")]
    assert len(line) == 1
    d2 = json.loads(line[0])
    assert d2["n_gpus"] == 2 and d2["config"]["global_envs"] == 512 and d2["scaling"] == "weak"
    # BASELINE configs[3] and [4] as slices of their GLOBAL batches (here divided by 64): both ranks' times, the
    # slowest rank, global env counts
    gc = d2["global_configs"]
    assert [g["workload"].split(" GLOBAL")[0] for g in gc] == ["formation_hd_env, 81 agents x 256 envs",
                                                               "formation_hd_env, 243 agents x 1024 envs"]
    for g, n_ag, n_env in zip(gc, (81, 243), (256, 1024)):
        assert g["scaling"] == "strong" and g["envs_per_gpu"] == n_env // 2 and len(g["per_rank_ms_per_step"]) == 2
        assert g["slowest_rank"] in (0, 1) and g["state_finite"] and g["test_scale_div"] == 64
        assert abs(g["env_steps_per_s"] - n_env / (g["ms_per_step"] * 1e-3)) < 2e-3 * g["env_steps_per_s"]
        assert abs(g["agent_steps_per_s"] - n_ag * g["env_steps_per_s"]) < 1e-3 * g["agent_steps_per_s"]
        # the denominator is the same global batch timed by rank 0 alone in the same run
        assert g["n1_same_run"] and g["n1_env_steps_per_s"] > 0 and 0.1 < g["scaling_efficiency_vs_n1"] < 3.0
    # default backend (nccl = RCCL) with more ranks than GPUs: RCCL cannot form a communicator over duplicate devices, so
    # bench.py keeps the timing barrier on gloo without trying (decided from the device count, same on every rank)
    out = _run(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", _free_port(), "bench.py", "--gpus", "2", "--steps", "20", "--warmup", "5", "--envs", "256",
                "--agents", "9", "--no-extra", "--min-timed-ms", "5"])
    line = [l for l in out.splitlines() if l.startswith("{")]
    assert len(line) == 1
    d3 = json.loads(line[0])
    assert d3["n_gpus"] == 2 and d3["config"]["timing_barrier"] == ("gloo" if torch.cuda.device_count() < 2 else "rccl")
    # without a launcher, `--gpus 2` starts its own ranks
    out = _run(["bench.py", "--gpus", "2", "--steps", "20", "--warmup", "5", "--envs", "256", "--agents", "9",
                "--backend", "gloo", "--no-extra", "--min-timed-ms", "5"])
    line = [l for l in out.splitlines() if l.startswith("{")]
    assert len(line) == 1 and json.loads(line[0])["n_gpus"] == 2


def test_bench_dump_outputs_are_the_same_from_run_to_run(tmp_path):
    """`bench.py --dump-outputs DIR` at the headline shape: what the last of the --steps timed steps computed, float32, a
    seeded sample of envs under 64 MB, bit for bit the same in two runs whose wall-clock prewarm differs (the env is put
    back to its state before the prewarm, so the timed steps never depend on the clock)."""
    import json
    import os
    dumps = []
    for prewarm in ("0", "300"):
        out = str(tmp_path / ("prewarm_" + prewarm))
        line = [l for l in _run(["bench.py", "--steps", "50", "--warmup", "10", "--no-extra", "--prewarm-ms", prewarm,
                                 "--dump-outputs", out]).splitlines() if l.startswith("{")]
        assert len(line) == 1
        d = json.loads(line[0])
        assert d["steps"] == 50 and d["timing"]["timed_steps"] == 50 and d["dump_outputs"]["dir"] == out
        files = sorted(os.listdir(out))
        assert files == sorted(k + ".npy" for k in ("obs", "reward", "indiv", "done", "pos", "vel"))
        assert sum(os.path.getsize(os.path.join(out, f)) for f in files) <= 64 * 10 ** 6
        dumps.append({f[:-4]: np.load(os.path.join(out, f)) for f in files})
    a, b = dumps
    n = a["obs"].shape[0]
    assert 0 < n < 4096 and a["obs"].shape == (n, 27, 162) and a["done"].shape == a["reward"].shape == (n, 27)
    for k in a:
        assert a[k].dtype == np.float32 and a[k].shape[0] == n
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert np.isfinite(a["obs"]).all() and np.isfinite(a["pos"]).all() and (a["obs"] != 0).any()


def test_bench_plain_run_is_the_headline_alone():
    """`bench.py --gpus 1 --steps N --warmup W` without --full: the headline workload timed as with --full (one series of
    exactly N steps), and nothing beside it - no other mode, no side timings of the headline launch, no counter passes,
    no other shapes, scenarios or CPU baselines."""
    import json
    import time
    t0 = time.perf_counter()
    line = [l for l in _run(["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"]).splitlines() if l.startswith("{")]
    elapsed = time.perf_counter() - t0
    assert len(line) == 1
    d = json.loads(line[0])
    assert d["metric"] == "env-steps/sec" and d["unit"] == "env-steps/s" and d["higher_is_better"] and d["dtype"] == "f32"
    assert d["steps"] == 20 and d["warmup"] == 5 and d["state_finite"] and d["value"] > 0
    t = d["timing"]
    assert t["timed_steps"] == 20 and t["blocks"] == 1
    assert abs(d["ms_per_step"] * 20 - t["block_ms_median"]) < 1e-3 * t["block_ms_median"] + 1e-5
    assert d["config"]["agents"] == 27 and d["config"]["envs_per_gpu"] == 4096 and d["config"]["mode"] == "rollout"
    for k in ("other_mode", "default_api", "rollout_cache_resident_buffer", "other_configs", "closed_loop_policy",
              "global_configs", "config1", "other_scenarios", "cpu_baseline", "cpu_baseline_other_shapes"):
        assert k not in d, k
    r = d["roofline"]
    assert "frac_unplaced" not in r and "traffic_live_error" not in r and "traffic_committed_profile" not in r
    assert not str(r.get("traffic_source") or "").startswith("live")
    # the --full run of the same arguments spends ~80 s beside its steps; the plain one a few seconds of set-up
    print("plain bench run: %.1f s" % elapsed)
    assert elapsed < 90, elapsed


def test_bench_many_ranks_share_the_gpu():
    """A rehearsal of the multi-GPU launch with as many ranks as this pool lets one GPU carry (its process guard allows six
    GPU processes of ours at once: this test's own + 4 ranks; the 8-rank case is the driver's to run on an 8-GPU node):
    `--gpus 4 --backend gloo --global-div 64` - four concurrent placement probes inside a quarter of the memory budget each
    (ranks_per_gpu = 4), four per-rank times, the global env counts, the solo N = 1 leg PLACED like the shards, no rank out of
    memory or timed out."""
    import json
    out = _run(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
                "--master-port", _free_port(), "bench.py", "--gpus", "4", "--steps", "20", "--warmup", "5", "--envs", "256",
                "--agents", "27", "--backend", "gloo", "--full", "--no-cpu-baseline", "--global-div", "64", "--min-timed-ms", "5"],
               timeout=600)
    line = [l for l in out.splitlines() if l.startswith("{")]
    assert len(line) == 1
    d = json.loads(line[0])
    assert d["n_gpus"] == 4 and d["config"]["global_envs"] == 1024 and d["config"]["ranks_per_gpu"] == -(-4 // torch.cuda.device_count())
    assert d["state_finite"] and d["value"] > 0
    gc = d["global_configs"]
    assert len(gc) == 2
    for g, n_env in zip(gc, (256, 1024)):
        assert "skipped" not in g, g
        assert g["envs_per_gpu"] == n_env // 4 and len(g["per_rank_ms_per_step"]) == 4 and all(x > 0 for x in g["per_rank_ms_per_step"])
        assert g["state_finite"] and g["n1_same_run"] and g["n1_env_steps_per_s"] > 0
        assert "n1_placement" in g and "scaling_denominator" in g         # the denominator is placed like the numerator
        if g["n1_placement"].get("probed"):
            assert g["scaling_efficiency_vs_n1_unplaced"] > 0


def test_c_abi_from_plain_cpp_without_python_or_torch(tmp_path):
    """examples/c_abi_rollout.cpp: hipMalloc'd buffers, the caller's stream, fg_reset_hd / fg_observe_hd /
    fg_rollout_hd / fg_step_hd through the header alone; checks its own results and prints throughput."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = os.path.join(root, "gym-formation_amd", "lib")
    exe = str(tmp_path / "c_abi_rollout")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O2", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "c_abi_rollout.cpp"), "-L", lib, "-lformation_hip",
                    "-Wl,-rpath," + lib, "-o", exe], check=True, capture_output=True, timeout=600)
    for args in (["9", "512", "100"], ["27", "256", "60"], ["10", "64", "40"]):
        out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "sanity ok" in out.stdout and "fg_rollout_hd" in out.stdout and "fg_step_hd" in out.stdout


def test_env_shards_reproduce_the_global_batch():
    """sharding.make_env_shard: the slices of 2 and of 3 ranks (sizes differ by one) concatenate to exactly what
    one process with the whole batch computes - reset streams follow the GLOBAL env index."""
    from formation_gym import sharding
    N, G = 9, 11
    whole, lo, hi = sharding.make_env_shard("formation_hd_env", N, G, seed=5, rank=0, world_size=1, local_rank=0)
    assert (lo, hi) == (0, G)
    obs_w = whole.reset().clone()
    act = torch.rand((G, N, 2), device="cuda") * 2 - 1
    step_w = [t.clone() for t in whole.step(act)[:3]]
    for world in (2, 3):
        parts = [sharding.make_env_shard("formation_hd_env", N, G, seed=5, rank=r, world_size=world, local_rank=0)
                 for r in range(world)]
        assert [p[1] for p in parts] + [G] == [p[1] for p in parts][:1] + [p[2] for p in parts]      # contiguous cover
        obs = torch.cat([e.reset() for e, _, _ in parts])
        assert torch.equal(obs, obs_w)
        outs = [e.step(act[l:h].contiguous())[:3] for e, l, h in parts]
        for k in range(3):
            assert torch.equal(torch.cat([o[k] for o in outs]), step_w[k])


def test_demo_driver_runs():
    out = _run(["gym-formation_amd/demo.py", "-n", "3", "--num-layer", "2", "--num-envs", "64", "--steps", "120"])
    assert "env-steps/s" in out
    out = _run(["gym-formation_amd/demo.py", "-s", "formation_hd_obs_env", "-n", "4", "-r", "--num-envs", "32", "--steps", "60"])
    assert "env-steps/s" in out


@pytest.mark.parametrize("name,opts", [("hd_n9_options", dict(max_speed=0.6, accel=3.0, walls=True)),
                                        ("hd_n27_walls", dict(walls=True))])
def test_world_options_teacher_forced(golden, name, opts):
    """max_speed, accel and walls (World features the reference scenarios leave off): state, rewards, done flags and the
    recorded observations of every teacher-forced step."""
    from formation_gym.core import Wall
    g = golden(name)
    T, B, N = g["acts"].shape[:3]
    env = _make(N, B)
    for a in env.world.agents:
        a.max_speed = opts.get("max_speed")
        a.accel = opts.get("accel")
    if opts.get("walls"):
        env.world.walls = [Wall(o, ax, ep, w) for (o, ax, ep, w) in O.GOLDEN_WALLS]
    prev_pos, prev_vel = g["pos0"], g["vel0"]
    for t in range(T):
        _load(env, prev_pos, prev_vel, g["ideal_shape"], g["ideal_vel"], np.full(B, t))
        obs, rew, done, info = env.step(torch.as_tensor(g["acts"][t]).cuda())
        pos, vel = env.world.get_state()
        np.testing.assert_allclose(_np(pos), g["pos"][t], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(vel), g["vel"][t], rtol=0, atol=ATOL)
        ok = g["cnt_margin"][t] > 1e-5
        np.testing.assert_allclose(_np(info["individual_reward"])[ok], g["indiv"][t][ok], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(rew)[ok, :, 0], g["shared"][t][ok], rtol=2e-6, atol=ATOL)
        np.testing.assert_array_equal(done.cpu().numpy(), g["done"][t])
        if (t + 1) in g["obs_steps"]:
            np.testing.assert_allclose(_np(obs), g["obs_t%d" % (t + 1)], rtol=0, atol=ATOL)
        prev_pos, prev_vel = g["pos"][t], g["vel"][t]
    if opts.get("max_speed"):
        assert float(torch.stack(env.world.get_state()[1:]).norm(dim=-1).max()) <= opts["max_speed"] * (1 + 1e-5)


@pytest.mark.parametrize("name", ["hd_n9_constants", "hd_n27_constants"])
def test_non_default_world_constants_teacher_forced(golden, name):
    """dt, damping, contact force / margin, agent mass and size, episode length away from the defaults
    (core.py:119-139), set on the World exactly as a reference user would; fixtures from the reference."""
    g = golden(name)
    T, B, N = g["acts"].shape[:3]
    env = _make(N, B)
    w = env.world
    w.dt, w.damping = float(g["world_dt"]), float(g["world_damping"])
    w.contact_force, w.contact_margin = float(g["world_contact_force"]), float(g["world_contact_margin"])
    w.world_length = env.world_length = int(g["world_world_length"])
    for a in w.agents:
        a.initial_mass = float(g["world_mass"])
        a.size = float(g["world_size"])
    prev_pos, prev_vel = g["pos0"], g["vel0"]
    for t in range(T):
        _load(env, prev_pos, prev_vel, g["ideal_shape"], g["ideal_vel"], np.full(B, t))
        obs, rew, done, info = env.step(torch.as_tensor(g["acts"][t]).cuda())
        pos, vel = env.world.get_state()
        np.testing.assert_allclose(_np(pos), g["pos"][t], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(vel), g["vel"][t], rtol=0, atol=ATOL)
        ok = g["cnt_margin"][t] > 1e-5
        np.testing.assert_allclose(_np(info["individual_reward"])[ok], g["indiv"][t][ok], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(rew)[ok, :, 0], g["shared"][t][ok], rtol=2e-6, atol=ATOL)
        np.testing.assert_array_equal(done.cpu().numpy(), g["done"][t])
        if (t + 1) in g["obs_steps"]:
            np.testing.assert_allclose(_np(obs), g["obs_t%d" % (t + 1)], rtol=0, atol=ATOL)
        prev_pos, prev_vel = g["pos"][t], g["vel"][t]
    # the same constants through a K-step rollout launch: bit-identical to single steps
    _load(env, g["pos0"], g["vel0"], g["ideal_shape"], g["ideal_vel"], np.zeros(B))
    acts = torch.as_tensor(g["acts"][:4]).cuda().contiguous()
    singles = []
    for t in range(4):
        o, r, d, _ = env.step(acts[t])
        singles.append((o.clone(), r.clone(), d.clone()))
    _load(env, g["pos0"], g["vel0"], g["ideal_shape"], g["ideal_vel"], np.zeros(B))
    ro = dict(obs=torch.empty((4, B, N, 6 * N), device="cuda"), reward=torch.empty((4, B, N), device="cuda"),
              done=torch.zeros((4, B, N), dtype=torch.uint8, device="cuda"))
    env.scenario.rollout_batch(env.world, acts, ro)
    for t in range(4):
        assert torch.equal(ro["obs"][t], singles[t][0])
        assert torch.equal(ro["reward"][t], singles[t][1][..., 0])
        assert torch.equal(ro["done"][t].bool(), singles[t][2])


@pytest.mark.parametrize("N,B,K,every", [(27, 33, 8, 1), (9, 20, 7, 2), (81, 3, 4, 1)])
def test_env_rollout_api_equals_step_calls(N, B, K, every):
    """`env.rollout(action_seq)` = K `env.step` calls bit for bit, episode ends and device resets included."""
    rs = np.random.RandomState(31 + N)
    st = O.reset_hd(rs.randint(0, 10000, B), N)
    acts = torch.as_tensor(rs.uniform(-1, 1, (K, B, N, 2)).astype(np.float32)).cuda()
    step0 = np.where(np.arange(B) % 2 == 0, 97, 3)
    a = _make(N, B); _load(a, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], step0)
    b = _make(N, B); _load(b, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], step0)
    for e in (a, b):
        e.scenario.seed(5); e.auto_reset = True
    obs, rew, done, info = b.rollout(acts, obs_every=every)
    assert obs.shape == (K // every, B, N, 6 * N) and rew.shape == (K, B, N, 1) and done.dtype == torch.bool
    for k in range(K):
        o, r, d, i = a.step(acts[k])
        if (k + 1) % every == 0:
            assert torch.equal(o, obs[k // every])
        assert torch.equal(r, rew[k]) and torch.equal(d, done[k])
        assert torch.equal(i["individual_reward"], info["individual_reward"][k])
    assert done.any() and not done.all()
    for x, y in zip(a.world.get_state(), b.world.get_state()):
        assert torch.equal(x, y)
    assert a.current_step == b.current_step == K and a._rng_offset == b._rng_offset
    # a second launch continues exactly where K more step calls would
    acts2 = torch.as_tensor(rs.uniform(-1, 1, (2, B, N, 2)).astype(np.float32)).cuda()
    o2 = b.rollout(acts2)[0]
    a.step(acts2[0]); o1 = a.step(acts2[1])[0]
    assert torch.equal(o1, o2[1])
    with pytest.raises(ValueError):
        b.rollout(acts[:, :1])
    # the vec-env adapter exposes the same launch
    from formation_gym.vec_env import FormationVecEnv
    va, vb = FormationVecEnv(_make(N, B)), FormationVecEnv(_make(N, B))
    for e in (va, vb):
        e.env.seed(9); e.reset(); e.env.scenario.seed(4)
    o_seq, r_seq, d_seq, _ = vb.rollout(acts)
    for k in range(K):
        o, r, d, _ = va.step(acts[k])
        assert torch.equal(o, o_seq[k]) and torch.equal(r, r_seq[k]) and torch.equal(d, d_seq[k])
    with pytest.raises(NotImplementedError):
        FormationVecEnv(_make(N, B), reset_mode="host").rollout(acts)


def test_empty_batch_is_a_noop():
    """num_envs = 0 (e.g. a rank that owns no envs when the batch is smaller than the world): every call
    succeeds and returns empty tensors of the right shapes."""
    N = 9
    env = _make(N, 0)
    env.seed(3)
    obs = env.reset()
    assert obs.shape == (0, N, 6 * N)
    o, r, d, i = env.step(torch.zeros((0, N, 2), device="cuda"))
    assert o.shape == (0, N, 6 * N) and r.shape == (0, N, 1) and d.shape == (0, N) and i["individual_reward"].shape == (0, N)
    o, r, d, i = env.rollout(torch.zeros((3, 0, N, 2), device="cuda"))
    assert o.shape == (3, 0, N, 6 * N) and r.shape == (3, 0, N, 1)
    torch.cuda.synchronize()


@pytest.mark.parametrize("N,B,K,L", [(27, 20, 47, 11), (9, 37, 60, 7), (81, 3, 23, 6), (3, 50, 64, 5)])
def test_one_launch_spanning_several_episodes(N, B, K, L):
    """K > several episode lengths: every env restarts more than once INSIDE one rollout launch; obs, rewards,
    dones and the reset draws equal K single-step launches bit for bit, and done fires exactly every L steps."""
    rs = np.random.RandomState(77 + N)
    st = O.reset_hd(rs.randint(0, 10000, B), N)
    acts = torch.as_tensor(rs.uniform(-1, 1, (K, B, N, 2)).astype(np.float32)).cuda()
    step0 = rs.randint(0, L, B)
    envs = []
    for _ in range(2):
        e = _make(N, B)
        e.world.world_length = e.world_length = L
        _load(e, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], step0)
        e.scenario.seed(21); e.auto_reset = True
        envs.append(e)
    a, b = envs
    obs, rew, done, info = b.rollout(acts)
    for k in range(K):
        o, r, d, i = a.step(acts[k])
        assert torch.equal(o, obs[k]) and torch.equal(r, rew[k]) and torch.equal(d, done[k])
    want_done = ((step0[None, :] + 1 + np.arange(K)[:, None]) % L) == 0          # [K, B]
    np.testing.assert_array_equal(done[:, :, 0].cpu().numpy(), want_done)
    assert want_done.sum(0).min() >= 2                                           # every env restarted at least twice
    assert torch.equal(a.scenario.ideal_shape, b.scenario.ideal_shape) and torch.equal(a.world.step_count, b.world.step_count)


def test_motor_noise_is_gaussian_with_the_requested_scale():
    """u_noise (core.py:232-233): device counter RNG, distributional parity only."""
    N, B = 9, 2048
    env = _make(N, B)
    st = O.reset_hd(1 + 1000 * np.arange(B), N)
    _load(env, st["pos"] * 3.0, st["vel"], st["ideal_shape"], st["ideal_vel"], st["step"])   # spread out: no contacts
    ref = _make(N, B)
    _load(ref, st["pos"] * 3.0, st["vel"], st["ideal_shape"], st["ideal_vel"], st["step"])
    for a in env.world.agents:
        a.u_noise = 0.5
    act = torch.zeros((B, N, 2), device="cuda")
    env.step(act); ref.step(act)
    dv = (env.world.get_state()[1] - ref.world.get_state()[1]) / 0.1          # = noise force (mass 1, dt 0.1)
    assert abs(float(dv.mean())) < 0.02 and abs(float(dv.std()) - 0.5) < 0.02
    env.step(act)
    dv2 = (env.world.get_state()[1] - ref.world.get_state()[1])
    assert float((dv2 / 0.1 - 0.75 * dv).std()) > 0.3                           # fresh noise every step


@pytest.mark.parametrize("N,B,K", [(27, 40, 6), (9, 70, 5), (3, 33, 4), (81, 3, 4)])
def test_rollout_with_auto_reset_equals_single_steps(N, B, K):
    """Episode ends inside a K-step launch: the pipelined rollout kernel must reset on device
    exactly like K single-step launches with the same RNG offsets (bit for bit)."""
    rs = np.random.RandomState(7 + N)
    st = O.reset_hd(rs.randint(0, 10000, B), N)
    acts = torch.as_tensor(rs.uniform(-1, 1, (K, B, N, 2)).astype(np.float32)).cuda()
    step0 = np.where(np.arange(B) % 3 == 0, 98, np.where(np.arange(B) % 3 == 1, 99, 5))   # mixed phases
    a = _make(N, B); _load(a, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], step0)
    b = _make(N, B); _load(b, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], step0)
    a.scenario.seed(11); b.scenario.seed(11)
    out = dict(obs=torch.empty((K, B, N, 6 * N), device="cuda"), reward=torch.empty((K, B, N), device="cuda"),
               indiv=torch.empty((K, B, N), device="cuda"),
               done=torch.zeros((K, B, N), dtype=torch.uint8, device="cuda"))
    b.scenario.rollout_batch(b.world, acts, out, auto_reset=True, rng_offset=1000)
    n_done = 0
    for k in range(K):
        a.scenario.step_batch(a.world, acts[k], a._out, auto_reset=True, rng_offset=1000 + k)
        assert torch.equal(a._out["obs"], out["obs"][k])
        assert torch.equal(a._out["reward"], out["reward"][k])
        assert torch.equal(a._out["done"], out["done"][k])
        n_done += int(a._out["done"][:, 0].sum())
    assert n_done >= B // 2                                   # episodes really ended inside the launch
    for x, y in zip(a.world.get_state(), b.world.get_state()):
        assert torch.equal(x, y)
    assert torch.equal(a.world.step_count, b.world.step_count)
    assert torch.equal(a.scenario.ideal_shape, b.scenario.ideal_shape)
    assert torch.equal(a.scenario.ideal_vel, b.scenario.ideal_vel)


@pytest.mark.parametrize("N,B", [(5, 33), (8, 17), (17, 9), (32, 5), (33, 6), (64, 3), (65, 4), (128, 2), (200, 2), (300, 1),
                                 (513, 1), (1024, 1)])
def test_generic_agent_counts_against_oracle(N, B):
    """Run-time-N kernels (every lane-group width and workgroup size), crowded so that contacts
    and collision counts occur, with the landmark-index outputs switched on."""
    rs = np.random.RandomState(1000 + N)
    st = O.reset_hd(rs.randint(0, 100000, B), N)
    st["pos"] *= 0.35
    st["vel"] = rs.uniform(-0.3, 0.3, (B, N, 2))
    act = rs.uniform(-1, 1, (B, N, 2)).astype(np.float32)
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    st = {k: (f32(v) if v.dtype != np.int32 else v) for k, v in st.items()}
    env = _make(N, B)
    env.enable_assignments(True)
    _load(env, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], st["step"])
    obs, rew, done, info = env.step(torch.as_tensor(act).cuda())
    new, out = O.step_hd(st, act.astype(np.float64))
    pos, vel = (_np(x) for x in env.world.get_state())
    np.testing.assert_allclose(pos, new["pos"], rtol=0, atol=ATOL)
    np.testing.assert_allclose(vel, new["vel"], rtol=0, atol=ATOL)
    r = O.reward_hd(pos, vel, st["ideal_shape"], st["ideal_vel"], O.HdParams())       # on the GPU's own state
    ok = r["cnt_margin"] > 1e-6
    np.testing.assert_allclose(_np(info["individual_reward"])[ok], r["indiv"][ok], rtol=0, atol=ATOL)
    np.testing.assert_allclose(_np(rew)[ok, :, 0], r["shared"][ok][:, None].repeat(N, 1), rtol=2e-6, atol=ATOL)
    np.testing.assert_allclose(_np(obs), O.observation_hd(pos, vel, st["ideal_shape"], st["ideal_vel"]), rtol=0, atol=2e-7)
    _check_indices(env._out["near_lm"].cpu().numpy(), r["near_lm"], r["gap_lm"], "near_lm")
    _check_indices(env._out["near_ag"].cpu().numpy(), r["near_ag"], r["gap_ag"], "near_ag")
    tie = r["hd_gap"].min(1) < 1e-6
    np.testing.assert_array_equal(env._out["hd_idx"].cpu().numpy()[~tie], r["hd_idx"][~tie])
    assert not done.any() and (env.world.step_count == 1).all()


def test_randomised_shapes_and_constants_against_oracle():
    """A seeded sweep over agent counts (specialised and run-time N), batch sizes, crowding and World constants,
    three free-running steps each, against the fp64 oracle with the same constants."""
    rs = np.random.RandomState(2024)
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    for case in range(24):
        N = int(rs.choice([3, 4, 5, 7, 9, 12, 16, 20, 27, 31, 40, 64, 81, 90]))
        B = int(rs.randint(1, 24))
        P = O.HdParams()
        P.dt = float(rs.uniform(0.03, 0.2)); P.damping = float(rs.uniform(0.05, 0.6))
        P.contact_force = float(rs.uniform(30, 200)); P.contact_margin = float(rs.uniform(5e-4, 5e-3))
        P.mass = float(rs.uniform(0.5, 3.0)); P.agent_size = float(rs.uniform(0.02, 0.1))
        P.world_length = int(rs.randint(2, 6))
        st = O.reset_hd(rs.randint(0, 100000, B), N)
        st["pos"] *= rs.uniform(0.2, 1.0)
        st["vel"] = rs.uniform(-0.5, 0.5, (B, N, 2))
        st = {k: (f32(v) if v.dtype != np.int32 else v) for k, v in st.items()}
        env = _make(N, B)
        w = env.world
        w.dt, w.damping, w.contact_force, w.contact_margin = P.dt, P.damping, P.contact_force, P.contact_margin
        w.world_length = env.world_length = P.world_length
        for a in w.agents:
            a.initial_mass, a.size = P.mass, P.agent_size
        _load(env, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], st["step"])
        for t in range(3):
            act = rs.uniform(-1, 1, (B, N, 2)).astype(np.float32)
            obs, rew, done, info = env.step(torch.as_tensor(act).cuda())
            st, out = O.step_hd(st, act.astype(np.float64), P)
            pos, vel = (_np(x) for x in env.world.get_state())
            # non-default constants (mass 0.5, contact force 200, dt 0.2 ...) drive speeds well above 1, where an fp32
            # ulp is proportionally larger: the 1e-5 bound is scaled by the largest speed in the batch (1 at the defaults)
            scale = max(1.0, float(np.abs(st["vel"]).max()))
            msg = "case %d N=%d B=%d t=%d" % (case, N, B, t)
            np.testing.assert_allclose(pos, st["pos"], rtol=0, atol=ATOL * scale, err_msg=msg)
            np.testing.assert_allclose(vel, st["vel"], rtol=0, atol=ATOL * scale, err_msg=msg)
            r = O.reward_hd(pos, vel, st["ideal_shape"], st["ideal_vel"], P)       # on the GPU's own fp32 state
            ok = r["cnt_margin"] > 1e-6
            np.testing.assert_allclose(_np(info["individual_reward"])[ok], r["indiv"][ok], rtol=0, atol=ATOL * scale, err_msg=msg)
            np.testing.assert_allclose(_np(rew)[ok, :, 0], r["shared"][ok][:, None].repeat(N, 1), rtol=2e-6, atol=ATOL * scale, err_msg=msg)
            np.testing.assert_allclose(_np(obs), O.observation_hd(pos, vel, st["ideal_shape"], st["ideal_vel"]), rtol=0, atol=5e-7 * scale, err_msg=msg)
            np.testing.assert_array_equal(done.cpu().numpy(), out["done"], err_msg=msg)
            st = dict(st, pos=pos, vel=vel)            # continue from the GPU's state: one-step comparisons, no chaotic drift


def test_entry_points_are_graph_capturable():
    """The C ABI enqueues on the caller's stream and never synchronises or allocates, so a
    sequence of env steps can be captured into a hipGraph (torch.cuda.CUDAGraph) and replayed."""
    N, B, K = 9, 128, 4
    rs = np.random.RandomState(3)
    st = O.reset_hd(rs.randint(0, 10000, B), N)
    acts = torch.as_tensor(rs.uniform(-1, 1, (K, B, N, 2)).astype(np.float32)).cuda()
    eager = _make(N, B); _load(eager, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], st["step"])
    graph_env = _make(N, B); _load(graph_env, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], st["step"])
    for k in range(K):
        eager.step(acts[k])
    want_obs = eager._out["obs"].clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for k in range(K):
                graph_env.scenario.step_batch(graph_env.world, acts[k], graph_env._out)
    torch.cuda.current_stream().wait_stream(side)
    # capture does not execute: state is still the initial one
    assert torch.equal(graph_env.world.step_count, torch.zeros_like(graph_env.world.step_count))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(graph_env._out["obs"], want_obs)
    for x, y in zip(eager.world.get_state(), graph_env.world.get_state()):
        assert torch.equal(x, y)
    assert (graph_env.world.step_count == K).all()


@pytest.mark.parametrize("N,B", [(3, 5), (9, 4), (27, 6), (81, 3), (243, 2), (100, 3)])
def test_device_mt19937_reset_is_bit_exact(N, B):
    """fg_reset_hd_mt continues each env's legacy NumPy stream on the GPU: three consecutive
    resets (N=243 needs several state regenerations per reset) equal the host path exactly."""
    import formation_gym
    dev_env = formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device="cuda:0")
    host_env = formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device="cuda:0")
    dev_env.seed(77); host_env.seed(77)
    dev_env.scenario.upload_mt_streams(dev_env.world)
    for rep in range(3):
        mask = None
        if rep == 1:                                   # masked reset: only some envs draw
            m = np.zeros(B, dtype=bool); m[::2] = True
            mask = torch.as_tensor(m.astype(np.uint8)).cuda()
            host_env.scenario.reset_world(host_env.world, env_mask=m)
        else:
            host_env.scenario.reset_world(host_env.world)
        dev_env.scenario.reset_mt(dev_env.world, mask)
        for x, y in zip(dev_env.world.get_state(), host_env.world.get_state()):
            assert torch.equal(x, y)
        assert torch.equal(dev_env.scenario.ideal_shape, host_env.scenario.ideal_shape)
        assert torch.equal(dev_env.scenario.ideal_vel, host_env.scenario.ideal_vel)
        assert torch.equal(dev_env.world.landmark_pos, host_env.world.landmark_pos)
    # and the very first reset reproduces the reference fixture stream
    g = load_golden_reset()
    if N in (9,):
        e = formation_gym.make_env("formation_hd_env", False, 9, num_envs=2, device="cuda:0")
        e.seed(7)
        from formation_gym.vec_env import FormationVecEnv
        obs = FormationVecEnv(e, reset_mode="device_mt").reset()
        np.testing.assert_allclose(_np(obs[0]), g["s7_n9_obs"], rtol=0, atol=1e-6)


def load_golden_reset():
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reset.npz")) as d:
        return {k: d[k] for k in d.files}


def test_vec_env_device_mt_matches_host_reset_mode():
    """Multi-episode rollout: 'device_mt' (no host round trip) == 'host' reset mode, bit for bit."""
    from formation_gym.vec_env import FormationVecEnv
    N, B, T = 9, 6, 7
    envs = []
    for mode in ("device_mt", "host"):
        e = _make(N, B)
        e.seed(21)
        v = FormationVecEnv(e, reset_mode=mode)
        v.reset()
        e.world.step_count.copy_(torch.tensor([97, 98, 99, 3, 98, 97], dtype=torch.int32))
        v.ts[:] = [97, 98, 99, 3, 98, 97]                      # the vec env's host mirror of the step counters just overwritten
        envs.append((e, v))
    rs = np.random.RandomState(5)
    for t in range(T):
        act = torch.as_tensor(rs.uniform(-1, 1, (B, N, 2)).astype(np.float32)).cuda()
        outs = [v.step(act) for (_, v) in envs]
        assert torch.equal(outs[0][0], outs[1][0])            # obs (reset obs where done)
        assert torch.equal(outs[0][1], outs[1][1])            # pre-reset reward
        assert torch.equal(outs[0][2], outs[1][2])            # pre-reset done
        assert torch.equal(envs[0][0].world.step_count, envs[1][0].world.step_count)


@pytest.mark.parametrize("N,B,L", [(27, 130, 4), (81, 12, 3), (10, 70, 5), (243, 3, 2)])
def test_vec_env_device_mt_single_launch_reset_at_other_sizes(N, B, L):
    """fg_reset_hd_mt_done (reset decided on the device + reset observation in the same launch) against the 'host' reset
    mode over several short episodes at mixed phases: observations, rewards, dones, final state and the MT19937 streams'
    continuation agree bit for bit."""
    from formation_gym.vec_env import FormationVecEnv
    envs = []
    phase = (np.arange(B) * 3) % L
    for mode in ("device_mt", "host"):
        e = _make(N, B)
        e.seed(33)
        v = FormationVecEnv(e, reset_mode=mode)
        v.reset()
        e.world.world_length = L
        e.world.step_count.copy_(torch.as_tensor(phase.astype(np.int32)))
        v.ts[:] = phase                                       # the vec env's host mirror of the step counters just overwritten
        envs.append((e, v))
    rs = np.random.RandomState(6)
    for t in range(3 * L + 1):
        act = torch.as_tensor(rs.uniform(-1, 1, (B, N, 2)).astype(np.float32)).cuda()
        outs = [v.step(act) for (_, v) in envs]
        for k in range(3):
            assert torch.equal(outs[0][k], outs[1][k]), (t, k)
    for x, y in zip(envs[0][0].world.get_state(), envs[1][0].world.get_state()):
        assert torch.equal(x, y)
    assert torch.equal(envs[0][0].world.step_count, envs[1][0].world.step_count)
    assert torch.equal(envs[0][0].scenario.ideal_shape, envs[1][0].scenario.ideal_shape)


def test_episode_statistics_match_oracle_over_100_steps():
    """Chaotic fp32 trajectories cannot match fp64 pointwise over an episode, but nothing may
    drift systematically: over 1024 envs x 100 steps the per-step batch means of reward, speed
    and collision penalty of the GPU rollout agree with the fp64 oracle to 1e-3 relative."""
    N, B, T = 27, 1024, 100
    st = O.reset_hd(1 + 1000 * np.arange(B), N)
    st["pos"] *= 0.5                                      # denser than the default: contacts matter
    acts = np.random.RandomState(0).uniform(-1, 1, (T, B, N, 2)).astype(np.float32)
    env = _make(N, B)
    _load(env, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], st["step"])
    out = dict(obs=None, reward=torch.empty((T, B, N), device="cuda"), indiv=torch.empty((T, B, N), device="cuda"),
               done=torch.zeros((T, B, N), dtype=torch.uint8, device="cuda"))
    out = {k: v for k, v in out.items() if v is not None}
    act_dev = torch.as_tensor(acts).cuda()
    gpu_speed = []
    for t0 in range(0, T, 20):
        chunk = {k: v[t0:t0 + 20] for k, v in out.items()}
        env.scenario.rollout_batch(env.world, act_dev[t0:t0 + 20], chunk)
        gpu_speed.append(float(torch.stack(env.world.get_state()[1:]).norm(dim=-1).mean()))
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    s = dict(st, pos=f32(st["pos"]), ideal_shape=f32(st["ideal_shape"]), ideal_vel=f32(st["ideal_vel"]))
    ref_rew, ref_pen, ref_speed = [], [], []
    for t in range(T):
        s, o = O.step_hd(s, acts[t].astype(np.float64))
        ref_rew.append(o["shared"].mean()); ref_pen.append(o["cnt"].mean())
        if (t + 1) % 20 == 0:
            ref_speed.append(np.sqrt((s["vel"] ** 2).sum(-1)).mean())
    gpu_rew = out["reward"][:, :, 0].double().mean(1).cpu().numpy()
    np.testing.assert_allclose(gpu_rew, np.array(ref_rew), rtol=1e-3, atol=1e-3)
    np.testing.assert_allclose(np.array(gpu_speed), np.array(ref_speed), rtol=1e-3)
    assert out["done"][-1].all() and not out["done"][-2].any()        # done flips exactly at step 100
    assert np.mean(ref_pen) > 0.01                                    # collisions did occur


def test_env_step_rebinds_when_inputs_or_world_constants_change():
    """env.step caches a pre-bound launch (pointers + FgParams).  A different action tensor, a changed
    World constant, enable_assignments and a non-default stream must each take effect on the next step."""
    N, B = 9, 33
    st = O.reset_hd(1 + 1000 * np.arange(B), N)
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    rs = np.random.RandomState(3)
    acts = [rs.uniform(-1, 1, (B, N, 2)).astype(np.float32) for _ in range(4)]
    env = _make(N, B)
    _load(env, st["pos"], st["vel"], st["ideal_shape"], st["ideal_vel"], st["step"])
    cur = dict(st, pos=f32(st["pos"]), ideal_shape=f32(st["ideal_shape"]), ideal_vel=f32(st["ideal_vel"]))

    def check(act, **world_options):
        nonlocal cur
        obs, rew, done, info = env.step(act)
        cur, out = O.step_hd(cur, _np(act), **world_options)
        pos, vel = (_np(x) for x in env.world.get_state())
        np.testing.assert_allclose(pos, cur["pos"], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(obs), out["obs"], rtol=0, atol=ATOL)
        cur = dict(cur, pos=pos, vel=vel)                 # teacher-force the oracle with the fp32 state
        return out

    a0, a1 = torch.as_tensor(acts[0]).cuda(), torch.as_tensor(acts[1]).cuda()
    check(a0)
    check(a0)                                             # same binding again
    assert len(env._launchers) == 1
    check(a1)                                             # another action buffer: second binding
    assert len(env._launchers) == 2
    a0.copy_(torch.as_tensor(acts[2]))                    # new contents in a bound buffer
    check(a0)
    for a in env.world.agents:                            # a World option switches kernels and constants
        a.max_speed = 0.3
    check(a1, max_speed=0.3)
    assert len(env._launchers) == 3
    env.enable_assignments(True)                          # new output buffers
    out = check(a1, max_speed=0.3)
    _check_indices(env._out["near_lm"].cpu().numpy(), out["near_lm"], out["gap_lm"], "near_lm")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # launch follows torch's current stream
        a3 = torch.as_tensor(acts[3]).cuda()
        n_before = len(env._launchers)
        check(a3, max_speed=0.3)
        assert len(env._launchers) == n_before + 1
    torch.cuda.current_stream().wait_stream(side)


@pytest.mark.parametrize("name,mode", [("act_onehot5_n3", "onehot5"), ("act_index_n9", "index"), ("act_argmax_n3", "argmax")])
def test_action_modes_match_reference_fixtures(golden, name, mode):
    """The non-default branches of _set_action (environment.py:187-216) through the reference-style
    list API (one env) and the batched tensor API (the same env replicated), teacher-forced."""
    import formation_gym
    g = golden(name)
    T, N = g["acts"].shape[0], g["pos0"].shape[0]

    def build(B):
        sc = formation_gym.load_scenario("formation_hd_env")
        world = sc.make_world(N, num_envs=B, device="cuda:0")
        if mode == "argmax":
            world.discrete_action = True
        env = formation_gym.MultiAgentEnv(world, sc.reset_world, sc.reward, sc.observation,
                                          discrete_action=(mode == "onehot5"))
        env.discrete_action_input = mode == "index"
        return env

    env1, envB = build(1), build(5)
    assert (getattr(env1.action_space[0], "n", -1) == 5) == (mode == "onehot5")
    for t in range(T):
        prev_pos, prev_vel = (g["pos0"], g["vel0"]) if t == 0 else (g["pos"][t - 1], g["vel"][t - 1])
        for env, B in ((env1, 1), (envB, 5)):
            _load(env, np.repeat(prev_pos[None], B, 0), np.repeat(prev_vel[None], B, 0),
                  np.repeat(g["ideal_shape"][None], B, 0), np.repeat(g["ideal_vel"][None], B, 0), np.full(B, t))
        # reference-style call
        if mode == "index":
            act_n = [int(a) for a in g["acts"][t]]
        else:
            act_n = [g["acts"][t, i].astype(np.float64).copy() for i in range(N)]
        obs_n, rew_n, done_n, info_n = env1.step(act_n)
        np.testing.assert_allclose(np.array(obs_n), g["obs"][t], rtol=0, atol=ATOL)
        np.testing.assert_allclose([r[0] for r in rew_n], g["shared"][t], rtol=2e-6, atol=ATOL)
        np.testing.assert_allclose([i["individual_reward"] for i in info_n], g["indiv"][t], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(env1.world.get_state()[0])[0], g["pos"][t], rtol=0, atol=ATOL)
        if mode != "index":
            np.testing.assert_array_equal(np.array(act_n), g["acts_after"][t])     # in-place effects on the caller's arrays
        # batched call
        dt = torch.int32 if mode == "index" else torch.float32
        act = torch.as_tensor(np.repeat(g["acts"][t][None], 5, 0)).to(device="cuda", dtype=dt)
        obs, rew, done, info = envB.step(act)
        np.testing.assert_allclose(_np(obs), np.repeat(g["obs"][t][None], 5, 0), rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(envB.world.get_state()[0]), np.repeat(g["pos"][t][None], 5, 0), rtol=0, atol=ATOL)
        if mode == "argmax":
            np.testing.assert_array_equal(_np(act)[0] * 5.0, g["acts_after"][t])   # one-hot written back


@pytest.mark.parametrize("mode", ["onehot5", "index", "argmax"])
def test_rollout_launch_in_the_discrete_action_modes(mode):
    """env.rollout(action_seq) in the non-default branches of _set_action (environment.py:194-215): the sequence is decoded to
    raw u in one launch, then K steps run in one launch - bit-identical to K env.step calls in the same mode."""
    import formation_gym
    N, B, K = 9, 300, 6

    def build():
        sc = formation_gym.load_scenario("formation_hd_env")
        world = sc.make_world(N, num_envs=B, device="cuda:0")
        if mode == "argmax":
            world.discrete_action = True
        env = formation_gym.MultiAgentEnv(world, sc.reset_world, sc.reward, sc.observation, discrete_action=(mode == "onehot5"))
        env.discrete_action_input = mode == "index"
        env.seed(3); env.reset()
        env.world.pos_x.mul_(0.3); env.world.pos_y.mul_(0.3)
        return env
    a, b = build(), build()
    gen = torch.Generator(device="cuda"); gen.manual_seed(7)
    if mode == "onehot5":
        seq = torch.rand((K, B, N, 5), device="cuda", generator=gen)
    elif mode == "index":
        seq = torch.randint(0, 5, (K, B, N), device="cuda", generator=gen, dtype=torch.int32)
    else:
        seq = torch.rand((K, B, N, 2), device="cuda", generator=gen) * 2 - 1
    seq_b = seq.clone()
    obs_seq, rew_seq, done_seq, info_seq = b.rollout(seq_b, out=False)
    for k in range(K):
        obs, rew, done, info = a.step(seq[k])
        assert torch.equal(obs, obs_seq[k]) and torch.equal(rew, rew_seq[k]) and torch.equal(done, done_seq[k])
        assert torch.equal(info["individual_reward"], info_seq["individual_reward"][k])
    for x, y in zip(a.world.get_state(), b.world.get_state()):
        assert torch.equal(x, y)
    if mode == "argmax":
        assert torch.equal(seq, seq_b)                   # both rewrote the caller's array as the one-hot (:213-215)
        assert set(np.unique(seq_b.cpu().numpy()).tolist()) <= {0.0, 1.0}
    with pytest.raises(ValueError):
        b.rollout(torch.zeros((K, B, N, 3), device="cuda"))


@pytest.mark.parametrize("N,B", [(81, 2048), (243, 8192), (243, 4099), (81, 16387)])     # 4099, 16387: the smallest batches of the pipelined single-step launch, ragged
def test_baseline_full_size_per_gpu_properties(N, B):
    """BASELINE configs 3 and 4 at their per-GPU batch (81 x 2048, 243 x 8192): size-independent
    properties checked on the device for EVERY env, the fp64 oracle on a sample of envs, and the same
    envs in a small batch bit for bit (the result of an env does not depend on the batch around it)."""
    dev = "cuda:0"
    env = _make(N, B)
    env.seed(5); env.reset()
    gen = torch.Generator(device=dev); gen.manual_seed(7)
    act = torch.rand((B, N, 2), generator=gen, device=dev) * 2 - 1
    pos0, vel0 = env.world.get_state()
    shape, ivel = env.scenario.ideal_shape.clone(), env.scenario.ideal_vel.clone()
    obs, rew, done, info = env.step(act)
    pos, vel = env.world.get_state()
    ind = info["individual_reward"]
    assert not bool(done.any())
    assert bool(torch.isfinite(obs).all()) and bool(torch.isfinite(rew).all())
    assert torch.allclose(ind.double().sum(1), rew[:, 0, 0].double(), rtol=2e-6, atol=1e-3)    # shared = sum of individuals
    assert bool((rew[:, :, 0] == rew[:, :1, 0]).all())
    assert bool((obs[:, :, 0:2] == vel).all())                                                 # own velocity
    assert bool((obs[:, :, 2 * N:4 * N - 2] == 0).all())                                       # comm block
    assert bool((obs[:, :, 4 * N - 2:6 * N - 2] == shape.reshape(B, 1, 2 * N)).all())           # ideal shape
    assert bool((obs[:, :, 6 * N - 2:] == ivel[:, None]).all())                                # ideal velocity
    # relative positions: row i holds p_j - p_i for j != i, in order; check two rows against the state exactly
    for i in (0, N // 2, N - 1):
        others = [j for j in range(N) if j != i]
        want = pos[:, others] - pos[:, i:i + 1]
        assert bool((obs[:, i, 2:2 * N].reshape(B, N - 1, 2) == want).all())
    # the fp64 oracle on a sample
    idx = np.random.RandomState(1).choice(B, 24, replace=False)
    st = dict(pos=_np(pos0)[idx], vel=_np(vel0)[idx], ideal_shape=_np(shape)[idx], ideal_vel=_np(ivel)[idx],
              step=np.zeros(len(idx), dtype=np.int32))
    new, out = O.step_hd(st, _np(act)[idx])
    np.testing.assert_allclose(_np(pos)[idx], new["pos"], rtol=0, atol=ATOL)
    ok = out["cnt_margin"] > 1e-5
    np.testing.assert_allclose(_np(ind)[idx][ok], out["indiv"][ok], rtol=0, atol=ATOL)
    np.testing.assert_allclose(_np(rew)[idx][ok], out["reward"][ok], rtol=2e-6, atol=ATOL)
    np.testing.assert_allclose(_np(obs[torch.as_tensor(idx, device=dev)]), out["obs"], rtol=0, atol=ATOL)
    # batch independence, bit for bit
    nb = 13
    env2 = _make(N, nb)
    sel = torch.as_tensor(idx[:nb], device=dev)
    _load(env2, _np(pos0[sel]), _np(vel0[sel]), _np(shape[sel]), _np(ivel[sel]), np.zeros(nb))
    obs2, rew2, _, info2 = env2.step(act[sel].contiguous())
    assert torch.equal(obs2, obs[sel]) and torch.equal(rew2, rew[sel])
    assert torch.equal(info2["individual_reward"], ind[sel])


def test_determinism_reentrancy_and_soak():
    """Same inputs -> same bits (two env objects, separate launches); two envs driven concurrently on
    two HIP streams give what they give alone (the C ABI is re-entrant and stream-ordered); and a
    1000-step auto-reset rollout stays finite and bounded (|v| <= 5 dt / damping per axis plus contacts)."""
    N, B, K = 27, 512, 20
    dev = "cuda:0"
    gen = torch.Generator(device=dev); gen.manual_seed(11)
    acts = torch.rand((K, B, N, 2), generator=gen, device=dev) * 2 - 1

    def fresh(seed):
        env = _make(N, B)
        env.seed(seed); env.reset()
        env.scenario._seed = seed
        return env

    def roll(env, n_chunks, stream=None):
        f = dict(dtype=torch.float32, device=dev)
        seq = dict(obs=torch.empty((K, B, N, 6 * N), **f), reward=torch.empty((K, B, N), **f),
                   indiv=torch.empty((K, B, N), **f), done=torch.zeros((K, B, N), dtype=torch.uint8, device=dev))
        tot = torch.zeros((), dtype=torch.float64, device=dev)
        for c in range(n_chunks):
            env.scenario.rollout_batch(env.world, acts, seq, auto_reset=True, rng_offset=c * K)
            tot = tot + seq["reward"].double().sum() + seq["obs"].double().abs().sum()
        return tot, seq

    # determinism
    a, b = fresh(3), fresh(3)
    ta, sa = roll(a, 3); tb, sb = roll(b, 3)
    assert torch.equal(sa["obs"], sb["obs"]) and torch.equal(sa["reward"], sb["reward"]) and bool(ta == tb)
    assert torch.equal(a.world.pos_x, b.world.pos_x) and torch.equal(a.world.step_count, b.world.step_count)
    # two streams at once == alone
    c, d = fresh(3), fresh(4)
    ref_d, _ = roll(fresh(4), 3)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        tc, sc = roll(c, 3)
    with torch.cuda.stream(s2):
        td, sd = roll(d, 3)
    torch.cuda.synchronize()
    assert bool(tc == ta) and bool(td == ref_d) and torch.equal(sc["obs"], sa["obs"])
    # soak: 50 launches x 20 steps = 10 episodes with auto-reset
    e = fresh(5)
    tot, seq = roll(e, 50)
    pos, vel = e.world.get_state()
    assert bool(torch.isfinite(tot)) and bool(torch.isfinite(pos).all()) and bool(torch.isfinite(vel).all())
    assert float(pos.abs().max()) < 25.0 and float(vel.abs().max()) < 8.0
    assert int(e.world.step_count.max()) < 100 and int(e.world.step_count.min()) >= 0
    assert int(seq["done"].sum()) == B * N                       # launch 50 ends at step 1000: every env is done once in it


def test_benchmark_flag_and_benchmark_data_match_reference(golden):
    """make_env(..., benchmark=True) (reference __init__.py:13-14): step() returns exactly what it returns without
    the flag (environment.py:130-133 forwards only a 'fail' key that benchmark_data never sets), and
    Scenario.benchmark_data (formation_hd_env.py:97-117) gives the reference's numbers for every agent."""
    import formation_gym
    g = golden("benchmark_n9")
    T, N = g["acts"].shape[:2]
    env = formation_gym.make_env("formation_hd_env", True, N)                    # reference signature, one env
    plain = formation_gym.make_env("formation_hd_env", False, N)
    assert env.info_callback is not None and plain.info_callback is None
    for e in (env, plain):
        e.world.set_state(g["pos0"][None], g["vel0"][None])
        e.scenario.set_formation(e.world, g["ideal_shape"][None], g["ideal_vel"][None])
        e.world.step_count.zero_()
    prev_pos, prev_vel = g["pos0"], g["vel0"]
    for t in range(T):
        for e in (env, plain):                                                  # teacher-forced
            e.world.set_state(prev_pos[None], prev_vel[None])
        act = [g["acts"][t, i].astype(np.float64) for i in range(N)]
        obs_n, rew_n, done_n, info_n = env.step([a.copy() for a in act])
        obs_p, rew_p, done_p, info_p = plain.step([a.copy() for a in act])
        assert all(sorted(i.keys()) == ["individual_reward"] for i in info_n)
        assert rew_n == rew_p and done_n == done_p and info_n == info_p
        assert all((a == b).all() for a, b in zip(obs_n, obs_p))
        np.testing.assert_allclose(rew_n[0][0], g["shared"][t], rtol=2e-6, atol=ATOL)
        for i, agent in enumerate(env.agents):
            bd = env._get_info(agent)
            assert set(bd) == {"reward", "collisions", "min_dists", "occupied_landmarks"}
            np.testing.assert_allclose(float(bd["reward"][0]), g["b_reward"][t, i], rtol=0, atol=ATOL)
            assert int(bd["collisions"][0]) == int(g["b_collisions"][t, i])
            np.testing.assert_allclose(float(bd["min_dists"][0]), g["b_min_dists"][t, i], rtol=2e-6, atol=ATOL)
            assert int(bd["occupied_landmarks"][0]) == int(g["b_occupied"][t, i])
        prev_pos, prev_vel = g["pos"][t], g["vel"][t]


def test_rank_processes_on_the_hip_path_reproduce_the_one_process_batch(tmp_path):
    """Multi-GPU plumbing with the REAL per-rank compute: 2 and 3 rank processes (sharing this box's one GPU), each
    stepping its slice of a global batch through libformation_hip under torch.distributed (gloo rendezvous, host-side
    gather), reproduce bit for bit what one process computes for the whole batch - reset streams by GLOBAL env index,
    device auto-resets keyed by global env, no collective on the data path."""
    from formation_gym import sharding
    N, G, K = 9, 37, 12
    whole, lo, hi = sharding.make_env_shard("formation_hd_env", N, G, seed=5, rank=0, world_size=1, local_rank=0)
    whole.auto_reset = True
    whole.reset()
    whole.world.step_count.copy_((torch.arange(G, dtype=torch.int32) * 7 % 100).cuda())
    gen = torch.Generator(); gen.manual_seed(123)
    acts = (torch.rand((K, G, N, 2), generator=gen) * 2 - 1).cuda()
    obs, rew, done, info = whole.rollout(acts)
    for ws in (2, 3):
        out = str(tmp_path / ("shards_%d.npz" % ws))
        _run(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ws), "--master-addr", "127.0.0.1",
              "--master-port", _free_port(), "tests/helpers/shard_worker.py", out, str(N), str(G), str(K)],
             env_extra={"HSA_ENABLE_IPC_MODE_LEGACY": "0"})
        r = np.load(out)
        assert r["slices"][0, 0] == 0 and r["slices"][-1, 1] == G and (r["slices"][1:, 0] == r["slices"][:-1, 1]).all()
        np.testing.assert_array_equal(r["obs_last"], obs[-1].cpu().numpy())
        np.testing.assert_array_equal(r["rew"], rew[..., 0].permute(1, 0, 2).cpu().numpy())
        np.testing.assert_array_equal(r["done"], done.permute(1, 0, 2).cpu().numpy().astype(np.uint8))
        np.testing.assert_array_equal(r["pos_x"], whole.world.pos_x.cpu().numpy())
        np.testing.assert_array_equal(r["shape"], whole.scenario.ideal_shape.cpu().numpy())
    assert done.any()


def test_vec_env_surface_matches_the_reference_loop(golden):
    """The vec-env surface an RL caller of the reference consumes (train/maddpg-v2/utils/env_wrappers.py:68-72, :113-122):
    stacked NumPy obs / rews / dones, infos per env, `ts`, the RESET observation with the finished step's reward / done -
    against fixture vec_env_n3, the reference's envs driven by DummyVecEnv.step_wait's loop body across an episode end.
    'host' reset mode: the reference's own MT19937 streams (seed + 1000 rank), so the reset observation is the reference's."""
    from formation_gym.vec_env import FormationVecEnv
    g = golden("vec_env_n3")
    T, B, N = g["acts"].shape[:3]
    env = _make(N, B)
    env.seed(int(g["seed"]))
    v = FormationVecEnv(env, reset_mode="host", numpy=True, infos="tuple")
    assert v.agent_types == list(g["agent_types"]) and v.get_spaces() == (env.observation_space, env.action_space)
    with pytest.raises(AttributeError, match="reset_task"):
        v.reset_task()
    obs = v.reset()
    assert isinstance(obs, np.ndarray) and obs.dtype == np.float64 and obs.shape == g["obs0"].shape
    np.testing.assert_allclose(obs, g["obs0"], rtol=0, atol=ATOL)
    W = int(g["world_length"])
    for t in range(T):
        obs, rews, dones, infos = v.step(g["acts"][t])           # NumPy in, NumPy out
        assert obs.dtype == np.float64 and rews.shape == (B, N, 1) and dones.dtype == np.bool_ and dones.shape == (B, N)
        assert isinstance(infos, tuple) and len(infos) == B and len(infos[0]) == N and sorted(infos[0][0]) == ["individual_reward"]
        np.testing.assert_array_equal(v.ts, g["ts"][t])
        np.testing.assert_array_equal(dones, g["dones"][t])
        # free-running fp32 against the fp64 reference: sparse 3-agent envs stay close; the step after the reset is fresh again
        tol = ATOL if (t % W) < 12 else 5e-4
        np.testing.assert_allclose(obs, g["obs"][t], rtol=0, atol=tol)
        np.testing.assert_allclose(rews, g["rews"][t], rtol=0, atol=10 * tol)
        np.testing.assert_allclose([[d["individual_reward"] for d in row] for row in infos], g["indiv"][t], rtol=0, atol=10 * tol)
    assert g["dones"][W - 1].all() and (g["ts"][W - 1] == 0).all()            # the episode end is inside the fixture
    # default return types: device tensors and one dict; `ts` also follows device-side resets without a read-back
    e2 = _make(N, B); e2.seed(3)
    v2 = FormationVecEnv(e2)
    v2.reset()
    e2.world.step_count.fill_(W - 2); v2.ts[:] = W - 2
    for t in range(3):
        o, r, d, i = v2.step(torch.zeros((B, N, 2), device="cuda"))
        assert torch.is_tensor(o) and isinstance(i, dict)
        np.testing.assert_array_equal(v2.ts, e2.world.step_count.cpu().numpy())
    assert (v2.ts == 1).all()
