"""Every draw of the device counter RNG against the NumPy Philox reference (tests/counter_rng.py): the device resets of
formation_hd_env and of the landmark scenarios, standalone and inside the step / rollout launches, the motor noise and the
communication noise.  The actor's exploration draws are held to the same reference in tests/test_gpu_actor_sample.py.

What is exact and what is bounded.  Positions, landmarks and ideal velocities are u_pm1 of a Philox word, exact in fp32: bit for
bit.  The ideal shape carries an fp32 sum over the env's lanes: `counter_rng.shape_bound`, per env, derived there.  Obstacles:
four fp32 roundings at magnitude <= 2.5, 4 * 2^-23 * 2.5.  Gaussian draws: `counter_rng.gauss_bound(r)` per draw, scaled by what
multiplies the draw, plus the fp32 roundings of the products that carry it (each test says which).

The inputs - seed 0x9E3779B97F4A7C15 (both key words set), env_index_base 3, offsets 5, 2^32 + 7 and 2^32 - 2 (steps 2 and 3 of
a K = 4 launch carry into the high word) - are the ones tests/test_counter_rng_cpu.py shows to tell the reference's mutants
apart.  The 64-bit seed does not go through `env.seed` (the host MT19937 streams are RandomState(seed + 1000 b)): the scenario's
seed and env_base attributes are set, from which every launch builds its FgParams.  Every env and every agent of every case is
compared.  Each test prints its measured maxima as shares of the bounds (`pytest -s`).  Run with `pytest -m gpu`.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-formation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import formation_oracle as O   # noqa: E402
from tests import counter_rng as R         # noqa: E402
from tests.counter_rng import BASE, K, OFFSETS, SEED  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
OBSTACLE_BOUND = 4 * 2.0 ** -23 * 2.5


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _t(x, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype).to(DEV)


def _exact(dev, ref, what):
    """fp32 device values == the fp64 reference rounded to fp32 (which the exact draws do not even round), bit for bit."""
    want = torch.as_tensor(np.asarray(ref).astype(np.float32))
    got = dev.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.equal(got, want), "%s: %d of %d values differ from the reference" % (what, int((got != want).sum()), want.numel())
    assert np.array_equal(want.numpy().astype(np.float64), np.asarray(ref)), "%s: the reference is not exact in fp32" % what


def _share(err, bound):
    return float((err / bound).max()) if err.size else 0.0


def _make(scenario, N, B, **agent_attrs):
    import formation_gym
    env = formation_gym.make_env(scenario, False, N, num_envs=B, device=DEV)
    env.scenario._seed = SEED                            # what `seed()` stores, without the host MT streams a 64-bit seed cannot key
    env.scenario.env_base = BASE
    for a in env.world.agents:
        for k, v in agent_attrs.items():
            setattr(a, k, v)
    return env


def _hd_state(env):
    w, sc = env.world, env.scenario
    return dict(pos=torch.stack((w.pos_x, w.pos_y), -1).clone(), vel=torch.stack((w.vel_x, w.vel_y), -1).clone(),
                shape=sc.ideal_shape.clone(), ivel=sc.ideal_vel.clone(), step=w.step_count.clone())


def _check_shape(shape_dev, ref, rows, N, what):
    """The ideal shape of envs `rows` within the derived per-env bound; returns the largest share of the bound used."""
    if not len(rows):
        return 0.0
    err = np.abs(_np(shape_dev)[rows] - ref["shape"][rows])
    bound = R.shape_bound(ref["raw"][rows], N)
    assert (err <= bound).all(), "%s: ideal shape off by %.3g of its bound" % (what, _share(err, bound))
    return _share(err, bound)


# ---------------------------------------------------------------------------------------------------------------------
# (a) formation_hd_env: the standalone reset
# ---------------------------------------------------------------------------------------------------------------------
def _sentinel(env):
    w, sc = env.world, env.scenario
    w.pos_x.fill_(7.0); w.pos_y.fill_(-7.0); w.vel_x.fill_(3.0); w.vel_y.fill_(-3.0)
    sc.ideal_shape.fill_(5.0); sc.ideal_vel.fill_(4.0); w.step_count.fill_(9)
    return _hd_state(env)


def _check_hd_reset(env, before, ref, mask, what):
    """Envs of `mask`: the reference's fresh state; the others: `before`, bit for bit."""
    N = env.num_agents
    st = _hd_state(env)
    inn, out = np.flatnonzero(mask), np.flatnonzero(~mask)
    _exact(st["pos"][inn], ref["pos"][inn], what + " positions")
    _exact(st["ivel"][inn], ref["ivel"][inn], what + " ideal velocity")
    assert not bool(st["vel"][inn].any()) and not bool(st["step"][inn].any()), what + ": velocities and step must be 0"
    for k in st:
        assert torch.equal(st[k][out], before[k][out]), "%s: %s of a masked-out env changed" % (what, k)
    return _check_shape(st["shape"], ref, inn, N, what)


@pytest.mark.parametrize("N,B", R.HD_RESET_SIZES)
def test_hd_reset_standalone(N, B):
    """`reset_device` with and without a mask at every lane-group width (4 ... 1024), the cross-wave sums above 64 lanes, a
    ragged last workgroup and more than one workgroup; the offset by value and split between rng_offset and the device counter."""
    env = _make("formation_hd_env", N, B)
    w, sc = env.world, env.scenario
    some = np.arange(B) % 3 != 1
    used, by_value = 0.0, {}
    for off in OFFSETS + (2 ** 32 + 1,):
        ref = R.hd_reset(SEED, BASE, B, N, off)
        for mask in (None, some):
            before = _sentinel(env)
            sc.reset_device(w, mask=None if mask is None else _t(mask, torch.uint8), rng_offset=off)
            what = "N=%d B=%d offset %#x%s" % (N, B, off, "" if mask is None else " masked")
            used = max(used, _check_hd_reset(env, before, ref, np.ones(B, bool) if mask is None else mask, what))
        by_value[off] = _hd_state(env)
    # the same sums with one part in the device counter (FgParams.rng_offset_dev): the high word there, and a carry out of the low one
    for part, counter in ((7, 2 ** 32), (2 ** 32 - 2, 3)):
        before = _sentinel(env)
        w.rng_counter = torch.full((1,), counter, dtype=torch.int64, device=DEV)
        sc.reset_device(w, mask=_t(some, torch.uint8), rng_offset=part)
        w.rng_counter = None
        st = _hd_state(env)
        for k in st:
            assert torch.equal(st[k], by_value[part + counter][k]), "rng_offset %#x + device counter %#x: %s differs" % (part, counter, k)
    if N <= 4:
        # while S = sum |raw| < 2 every partial sum is a multiple of 2^-23 below 2, hence exact: the bare 2^-24 (shape_bound)
        ref = R.hd_reset(SEED, BASE, B, N, OFFSETS[0])
        sc.reset_device(w, rng_offset=OFFSETS[0])
        small = np.broadcast_to(np.abs(ref["raw"]).sum(1, keepdims=True) < 2.0, ref["raw"].shape)
        assert small.sum() >= 0.25 * small.size
        assert (np.abs(_np(sc.ideal_shape) - ref["shape"])[small] <= 2.0 ** -24).all()
    print("counter_rng measured: hd reset N=%d shape error %.3f of its bound (G = %d)" % (N, used, R.lane_group(N)))


# ---------------------------------------------------------------------------------------------------------------------
# (b) formation_hd_env: the reset inside the launches
# ---------------------------------------------------------------------------------------------------------------------
def _describe(env, K_, per_layer=0, scenario=None):
    from formation_gym import _native
    sc = env.scenario
    p = sc.params(env.world, auto_reset=True)
    buf = ctypes.create_string_buffer(1024)
    _native.check(_native.load().fg_describe_launch(p, scenario, env.num_envs, env.num_agents, K_, per_layer, 1, 0, buf, len(buf)))
    return buf.value.decode()


def _zero_actor(N):
    from tests.actor_testlib import scaled_mlp
    return scaled_mlp(6 * N, 64, False, 0, 0.0)


def _finish_steps(B, K_):
    """Per env the step of the launch its episode ends at (b % 4: 0, 2, K - 1, never), -1 where that is beyond the launch."""
    fin = np.array([0, 2, K - 1, -1])[np.arange(B) % 4]
    return np.where(fin < K_, fin, -1)


def _launch_hd(env, kind, K_, rbase, acts):
    """One launch of `kind` at base offset rbase -> observations [K_, B, N, 6N]."""
    env._rng_offset = rbase - 1                          # the next launch draws at rbase
    assert env._launch_rng_offset() == rbase
    if kind == "step":
        obs = env.step(acts[0])[0].clone()[None]
    elif kind == "rollout":
        obs = env.rollout(acts, out=False)[0]
    elif kind == "policy":
        obs = env.rollout_policy(K_, 3, out=False)[0]
    else:
        obs = env.rollout_actor(K_, _zero_actor(env.num_agents), out=False)[0]
    torch.cuda.synchronize()
    return obs


def _hd_launch_case(env, kind, rbase, start):
    """Load `start`, run one launch whose episodes end at steps 0, 2, K - 1 or not at all, compare every env."""
    N, B = env.num_agents, env.num_envs
    w, sc = env.world, env.scenario
    W = int(w.world_length)
    K_ = 1 if kind == "step" else K
    fin = _finish_steps(B, K_)
    w.set_state(start["pos"], np.zeros((B, N, 2)))
    sc.set_formation(w, start["shape"], start["ivel"])
    w.step_count.copy_(_t(np.where(fin >= 0, W - 1 - fin, 5), torch.int32))
    before = _hd_state(env)
    gen = torch.Generator(device="cuda"); gen.manual_seed(N)
    acts = ((torch.rand((K_, B, N, 2), generator=gen, device="cuda") * 2 - 1) * 0.3).contiguous()
    obs = _launch_hd(env, kind, K_, rbase, acts)
    assert obs.shape == (K_, B, N, 6 * N)
    st = _hd_state(env)
    used = 0.0
    offs = R.launch_offsets(rbase, K_)
    for k in sorted(set(fin[fin >= 0])):
        rows = np.flatnonzero(fin == k)
        ref = R.hd_reset(SEED, BASE, B, N, offs[k])
        what = "%s N=%d B=%d rbase %#x, episodes ending at step %d" % (kind, N, B, rbase, k)
        _exact(st["ivel"][rows], ref["ivel"][rows], what + ": ideal velocity")
        used = max(used, _check_shape(st["shape"], ref, rows, N, what))
        assert torch.equal(st["step"][rows].cpu(), torch.full((len(rows),), K_ - 1 - k, dtype=torch.int32)), what
        if k == K_ - 1:
            _exact(st["pos"][rows], ref["pos"][rows], what + ": positions")
            assert not bool(st["vel"][rows].any()), what + ": velocities"
        # the observation that comes back with the finished step is the fresh state's
        want = O.observation_hd(ref["pos"][rows], np.zeros((len(rows), N, 2)), ref["shape"][rows], ref["ivel"][rows])
        np.testing.assert_allclose(_np(obs[k])[rows], want, rtol=0, atol=1e-6, err_msg=what)
    rows = np.flatnonzero(fin < 0)
    assert len(rows) or B < 4
    for key in ("shape", "ivel"):
        assert torch.equal(st[key][rows], before[key][rows]), "%s: %s of an env that did not finish changed" % (kind, key)
    assert torch.equal(st["step"][rows], before["step"][rows] + K_)
    return used


def _expected_kernel(kind, N, B, opts):
    if opts:
        return r"step_kernel<(0|%d),\d+,\d+,\d+,1,1," % N   # IDX, OPTS: the World-option instantiation, its K-loop for K > 1
    if kind == "step" or (kind == "rollout" and N > 64):    # (open loop, > 64 agents, <= 512 envs: step_kernel's K-loop)
        return r"step_kernel<%d,\d+,\d+,\d+,0,0," % N
    if N > 64:
        return r"rollout_kernel_wide<%d,\d+,\d+,\d+,3," % N
    if N == 3 and B >= 32768:
        return r"hd_lane_kernel<3,0,1>"
    return r"rollout_kernel<%d,\d+,\d+,\d+,\d+,\d+,%d," % (N, 3 if kind == "policy" else 0)


HD_LAUNCHES = ([(kind, N, B, False) for N, B in R.HD_LAUNCH_SIZES for kind in ("step", "rollout", "policy", "actor")] +
               [(kind, N, B, True) for N, B in R.HD_OPTION_SIZES for kind in ("step", "rollout", "actor")] +     # (17, 200: no 3^L hierarchy)
               [("rollout", 3, 32768, False)])             # the one-env-per-lane kernel is taken from 32768 envs up


@pytest.mark.parametrize("kind,N,B,opts", HD_LAUNCHES, ids=lambda v: str(v))
def test_hd_reset_inside_launches(kind, N, B, opts):
    """The fused auto-reset of `step`, `rollout` (K = 4), the closed-loop `rollout_policy` and `rollout_actor` (a zero actor):
    hd_lane_kernel, rollout_kernel, rollout_kernel_wide, the actor body, step_kernel and - with a World option set -
    step_kernel<OPTS> and its K-loop.  Episodes end at step 0, 2, K - 1 of the launch or not at all."""
    env = _make("formation_hd_env", N, B, **(dict(max_speed=1.5) if opts else {}))
    env.auto_reset = True
    if kind == "actor":
        path = env.actor_path(_zero_actor(N))
        assert path == ("fused" if N in (3, 9, 27) and not opts else "host"), path
        if path == "host":
            assert re.search(_expected_kernel("step", N, B, opts), _describe(env, 0))
    else:
        text = _describe(env, 0 if kind == "step" else K, 3 if kind == "policy" else 0)
        assert re.search(_expected_kernel(kind, N, B, opts), text), text
    start = R.hd_reset(11, 0, B, N, 1000)                  # any state: the reference at another key
    start["pos"] = start["pos"] * 0.5
    used = 0.0
    for rbase in (OFFSETS if B < 32768 else OFFSETS[2:]):
        used = max(used, _hd_launch_case(env, kind, rbase, start))
    print("counter_rng measured: hd %s N=%d shape error %.3f of its bound" % (kind, N, used))


@pytest.mark.parametrize("N,B", [(9, 37), (27, 13)])
def test_hd_launch_offset_split_with_the_device_counter(N, B):
    """`use_device_rng_counter`: the launch's base offset is rng_offset + the device counter.  With 2^32 - 3 in the counter and 1
    by value the K = 4 launch draws what it draws at 2^32 - 2 by value, the carry included: state and observations bit for bit."""
    res = []
    for split in (False, True):
        env = _make("formation_hd_env", N, B)
        env.auto_reset = True
        w, sc = env.world, env.scenario
        start = R.hd_reset(11, 0, B, N, 1000)
        fin = _finish_steps(B, K)
        w.set_state(start["pos"] * 0.5, np.zeros((B, N, 2)))
        sc.set_formation(w, start["shape"], start["ivel"])
        w.step_count.copy_(_t(np.where(fin >= 0, int(w.world_length) - 1 - fin, 5), torch.int32))
        env._rng_offset = OFFSETS[2] - 1
        if split:
            env.use_device_rng_counter(True)
            assert env._launch_rng_offset() == 1 and int(w.rng_counter.item()) == OFFSETS[2] - 1
        acts = torch.zeros((K, B, N, 2), device=DEV)
        obs = env.rollout(acts, out=False)[0].clone()
        res.append((obs, _hd_state(env)))
    assert torch.equal(res[0][0], res[1][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k
    ref = R.hd_reset(SEED, BASE, B, N, OFFSETS[2] + K - 1)
    rows = np.flatnonzero(fin == K - 1)
    _exact(res[1][1]["pos"][rows], ref["pos"][rows], "positions at 2^32 + 1 through the device counter")


# ---------------------------------------------------------------------------------------------------------------------
# (c) the landmark scenarios
# ---------------------------------------------------------------------------------------------------------------------
def _descriptor(env):
    sc = env.scenario
    return sc.descriptor() if hasattr(sc, "descriptor") else sc._descriptor(env.world)      # (basic_formation_env builds its own)


def _scn_state(env):
    w = env.world
    return dict(pos=torch.stack((w.pos_x, w.pos_y), -1).clone(), vel=torch.stack((w.vel_x, w.vel_y), -1).clone(),
                lm=w.landmark_pos.clone(), opos=w.obstacle_pos.clone(), ovel=w.obstacle_vel.clone(), step=w.step_count.clone())


def _check_scn_fresh(st, ref, rows, M, sc, what, agents=True):
    used = 0.0
    _exact(st["lm"][rows], ref["lm"][rows], what + ": landmarks")
    if agents:
        _exact(st["pos"][rows], ref["pos"][rows], what + ": agents")
        assert not bool(st["vel"][rows].any()) and not bool(st["step"][rows].any()), what
        if M:
            err = np.abs(_np(st["opos"])[rows] - ref["opos"][rows])
            assert (err <= OBSTACLE_BOUND).all(), "%s: obstacles off by %.3g" % (what, err.max())
            used = err.max() / OBSTACLE_BOUND if err.size else 0.0
            want = torch.tensor(sc.OBSTACLE_VEL, device=DEV).expand(len(rows), M, 2)
            assert torch.equal(st["ovel"][rows], want), what + ": obstacle velocities"
    return used


@pytest.mark.parametrize("scenario,kind,N,B,L,M", R.SCN_CASES)
def test_landmark_resets(scenario, kind, N, B, L, M):
    """`reset_device` (masked and not), and the fused auto-reset of the one-env-per-lane kernels and of the run-time-count kernel
    (`kernel_variant = 1`; 70 agents take it anyway), single steps and K = 4 launches."""
    env = _make(scenario, N, B)
    w, sc = env.world, env.scenario
    d = _descriptor(env)
    assert (d.num_landmarks, d.num_obstacles) == (L, M)
    some = np.arange(B) % 3 != 1
    used = 0.0
    for off in OFFSETS:
        ref = R.scn_reset(SEED, BASE, B, N, off, L, M)
        for mask in (None, some):
            for t in (w.pos_x, w.pos_y, w.vel_x, w.vel_y, w.landmark_pos, w.obstacle_pos, w.obstacle_vel):
                t.fill_(7.0)
            w.step_count.fill_(9)
            before = _scn_state(env)
            sc.reset_device(w, mask=None if mask is None else _t(mask, torch.uint8), rng_offset=off)
            st = _scn_state(env)
            inn = np.flatnonzero(np.ones(B, bool) if mask is None else mask)
            out = np.flatnonzero(np.zeros(B, bool) if mask is None else ~mask)
            used = max(used, _check_scn_fresh(st, ref, inn, M, sc, "%s reset_device offset %#x" % (scenario, off)))
            for k in st:
                assert torch.equal(st[k][out], before[k][out]), "%s of a masked-out env changed" % k
    env.auto_reset = True
    W = int(w.world_length)
    start = R.scn_reset(11, 0, B, N, 1000, L, M)
    for variant, K_ in ((0, K), (1, K), (0, 1)):
        sc.kernel_variant = variant
        text = _describe(env, K_, scenario=_descriptor(env))
        lane = variant == 0 and N < 64
        assert ("scn_lane_kernel<" in text) == lane and ("scn_kernel<" in text) != lane, text
        fin = _finish_steps(B, K_)
        for rbase in OFFSETS:
            w.set_state(start["pos"], np.zeros((B, N, 2)))
            w.landmark_pos.copy_(_t(start["lm"]))
            if M:
                w.obstacle_pos.copy_(_t(start["opos"]))
                w.obstacle_vel.copy_(torch.tensor(sc.OBSTACLE_VEL, device=DEV).expand(B, M, 2))
            w.step_count.copy_(_t(np.where(fin >= 0, W - 1 - fin, 5), torch.int32))
            before = _scn_state(env)
            env._rng_offset = rbase - 1
            acts = torch.zeros((K_, B, N, 2), device=DEV)
            if K_ == 1:
                env.step(acts[0])
            else:
                env.rollout(acts, out=False)
            torch.cuda.synchronize()
            st = _scn_state(env)
            offs = R.launch_offsets(rbase, K_)
            for k in sorted(set(fin[fin >= 0])):
                rows = np.flatnonzero(fin == k)
                ref = R.scn_reset(SEED, BASE, B, N, offs[k], L, M)
                what = "%s variant %d K=%d rbase %#x step %d" % (scenario, variant, K_, rbase, k)
                used = max(used, _check_scn_fresh(st, ref, rows, M, sc, what, agents=k == K_ - 1))
                assert torch.equal(st["step"][rows].cpu(), torch.full((len(rows),), K_ - 1 - k, dtype=torch.int32)), what
            rows = np.flatnonzero(fin < 0)
            assert torch.equal(st["lm"][rows], before["lm"][rows]) and torch.equal(st["step"][rows], before["step"][rows] + K_)
    print("counter_rng measured: %s N=%d obstacle error %.3f of its bound" % (scenario, N, used))


# ---------------------------------------------------------------------------------------------------------------------
# (d) motor noise
# ---------------------------------------------------------------------------------------------------------------------
U_NOISE, MASS = 0.5, 2.0
DT32 = float(np.float32(0.1))                            # FgParams.dt is fp32


def _spread(env):
    """Agents 2 apart on a line (and everything else far away): no contact force survives the cut-off, velocities 0."""
    w = env.world
    B, N = env.num_envs, env.num_agents
    pos = np.zeros((B, N, 2))
    pos[..., 0] = 2.0 * np.arange(N) - N
    pos[..., 1] = 40.0 * (np.arange(B)[:, None] % 2)
    w.set_state(pos, np.zeros((B, N, 2)))
    w.step_count.zero_()
    if getattr(w, "num_obstacles", 0):
        w.obstacle_pos.fill_(500.0)


def _noise_velocities(env, K_, rbase):
    _spread(env)
    env._rng_offset = rbase - 1
    acts = torch.zeros((K_,) + tuple(env._act.shape), device=DEV)
    if K_ == 1:
        env.step(acts[0])
    else:
        env.rollout(acts, out=False)
    torch.cuda.synchronize()
    return _np(env.world.get_state()[1])


def _check_motor(env, u_noise, what):
    """Velocities after K_ noisy steps from rest against the fp64 recurrence v <- (1 - damping) v + u_noise n_k / mass dt with
    the reference draws n_k; per component and per step taken the bound is scale (7e-7 r + 1e-7) for the draw (scale = u_noise
    dt / mass, which multiplies it) + 4 * 2^-24 |v| for the fp32 products and the sum of the update."""
    B, N = env.num_envs, env.num_agents
    u = np.broadcast_to(np.asarray(u_noise, dtype=np.float64), (N,))[None, :, None]
    used = 0.0
    for K_ in (1, K):
        for rbase in OFFSETS:
            got = _noise_velocities(env, K_, rbase)
            v, bound = np.zeros((B, N, 2)), np.zeros((B, N, 2))
            for off in R.launch_offsets(rbase, K_):
                n = R.motor_noise(SEED, BASE, B, N, off)
                r = np.sqrt((n * n).sum(-1, keepdims=True))
                v = (1.0 - env.world.damping) * v + u * n / MASS * DT32
                bound = bound + u * DT32 / MASS * R.gauss_bound(r) + 4 * 2.0 ** -24 * np.abs(v)
            err = np.abs(got - v)
            ok = err <= bound
            assert ok.all(), "%s K=%d rbase %#x: %d of %d velocities beyond the bound, worst %.3g of it" % (
                what, K_, rbase, int((~ok).sum()), ok.size, _share(err[bound > 0], bound[bound > 0]))
            quiet = np.flatnonzero(u.reshape(-1) == 0.0)
            assert not got[:, quiet].any(), what + ": an agent without noise moved"
            used = max(used, _share(err[bound > 0], bound[bound > 0]))
    return used


@pytest.mark.parametrize("N,B", R.MOTOR_SIZES)
@pytest.mark.parametrize("per_agent", [False, True], ids=["uniform", "per-agent"])
def test_motor_noise_hd(N, B, per_agent):
    """step_kernel<OPTS>, single steps and its K-loop: u_noise as the World-wide scalar, and as a column of agent_props with
    one agent at 0 (velocity exactly 0) and one at half the scale."""
    twin = _make("formation_hd_env", N, B, initial_mass=MASS)
    for K_ in (1, K):
        assert not _noise_velocities(twin, K_, 5).any(), "the noiseless twin moves: a contact force survives"
    env = _make("formation_hd_env", N, B, initial_mass=MASS, u_noise=U_NOISE)
    u = U_NOISE
    if per_agent:
        u = np.full(N, U_NOISE)
        u[1], u[N - 1] = 0.0, 0.5 * U_NOISE
        for a, x in zip(env.world.agents, u):
            a.u_noise = float(x) or None
        assert env.scenario.params(env.world).agent_props
    for K_ in (0, K):
        assert re.search(_expected_kernel("step", N, B, True), _describe(env, K_)), _describe(env, K_)
    used = _check_motor(env, u, "hd N=%d B=%d%s" % (N, B, " per-agent" if per_agent else ""))
    print("counter_rng measured: motor noise hd N=%d %s %.3f of its bound" % (N, "per-agent" if per_agent else "uniform", used))


@pytest.mark.parametrize("scenario,variant", [("basic_formation_env", 0), ("formation_hd_partial_range_env", 0),
                                              ("formation_hd_partial_range_env", 1)])
def test_motor_noise_landmark(scenario, variant):
    """The one-env-per-lane step (fg_scn_lane_step.inc) and scn_kernel (`kernel_variant = 1`), 3 agents x 37 envs, single steps
    and K = 4 launches.  (basic_formation_env's single step has no variant to choose: its lane kernel only.)"""
    N, B = 3, 37
    twin = _make(scenario, N, B, initial_mass=MASS)
    env = _make(scenario, N, B, initial_mass=MASS, u_noise=U_NOISE)
    for e in (twin, env):
        e.scenario.kernel_variant = variant
        e.world.landmark_pos.fill_(300.0)
    for K_ in (1, K):
        text = _describe(env, K_, scenario=_descriptor(env))
        assert ("scn_lane_kernel<" in text) == (variant == 0) and ("scn_kernel<" in text) == (variant == 1), text
        assert not _noise_velocities(twin, K_, 5).any(), "the noiseless twin moves"
    used = _check_motor(env, U_NOISE, "%s N=3 variant %d" % (scenario, variant))
    print("counter_rng measured: motor noise %s variant %d %.3f of its bound" % (scenario, variant, used))


# ---------------------------------------------------------------------------------------------------------------------
# (e) communication noise
# ---------------------------------------------------------------------------------------------------------------------
def test_comm_noise():
    """update_comm_kernel (dim_c = 2) and update_comm_dim_kernel (dim_c 1, 2, 3, 5): a silent agent reads zeros, a noiseless one its
    action.c exactly, the others action.c + c_noise n within c_noise (7e-7 r + 1e-7) for the draw + 2^-24 |c| for the sum (the
    scales are powers of two: the product with the draw is exact).  Pair 0 of any width is the dim_c = 2 kernel's draw."""
    from formation_gym import _native
    lib = _native.load()
    N, B = R.COMM_SIZE
    env = _make("formation_hd_env", N, B)
    w = env.world
    c_noise = np.array([-1.0, 0.0, 0.25, 0.5, 0.25])       # silent | noiseless | noisy
    for a, c in zip(w.agents, c_noise):
        a.silent = bool(c < 0)
        a.c_noise = float(c) if c > 0 else None
    props = w.agent_props()
    assert props is not None and np.array_equal(_np(props[:, 5]), c_noise)
    used = 0.0
    for off in OFFSETS + (2 ** 32 + 1,):
        p = w.native_params(seed=SEED, rng_offset=off, scripted_ok=True)
        p.agent_props, p.env_index_base = props.data_ptr(), BASE
        pair0 = None
        for dim_c, entry in [(2, "fg_update_comm")] + [(d, "fg_update_comm_dim") for d in R.COMM_DIMS]:
            gen = torch.Generator(device="cuda"); gen.manual_seed(dim_c)
            act = (torch.rand((B, N, dim_c), generator=gen, device="cuda") * 2 - 1).contiguous()
            comm = torch.full((B, N, dim_c), 7.0, device=DEV)
            lead = (p, B, N) if entry == "fg_update_comm" else (p, B, N, dim_c)
            _native.check(getattr(lib, entry)(*lead, act.data_ptr(), comm.data_ptr(), _native.current_stream(DEV)))
            torch.cuda.synchronize()
            assert not bool(comm[:, 0].any()), "the silent agent's state.c must read zeros"
            assert torch.equal(comm[:, 1], act[:, 1]), "the noiseless agent's state.c must be its action.c"
            n = R.comm_noise(SEED, BASE, B, N, off, dim_c)[:, 2:]
            s = c_noise[None, 2:, None]
            want = _np(act)[:, 2:] + s * n
            pairs = (dim_c + 1) // 2
            full = R.comm_noise(SEED, BASE, B, N, off, 2 * pairs)[:, 2:].reshape(B, N - 2, pairs, 2)
            r = np.repeat(np.sqrt((full * full).sum(-1)), 2, axis=-1)[..., :dim_c]       # the radius of each component's own draw
            bound = s * R.gauss_bound(r) + 2.0 ** -24 * np.abs(want)
            err = np.abs(_np(comm)[:, 2:] - want)
            assert (err <= bound).all(), "%s dim_c=%d offset %#x: worst %.3g of the bound" % (entry, dim_c, off, _share(err, bound))
            used = max(used, _share(err, bound))
            if entry == "fg_update_comm":
                pair0 = (act, comm.clone())
            elif dim_c == 2:
                # the same actions (same generator seed): update_comm_dim_kernel at 2 is update_comm_kernel, bit for bit
                assert torch.equal(act, pair0[0]) and torch.equal(comm, pair0[1])
            else:
                # pair 0 of another width draws what the dim_c = 2 kernel draws: the same fp32 noise, re-added to other actions
                act2 = torch.zeros((B, N, 2), device=DEV)
                comm2 = torch.empty((B, N, 2), device=DEV)
                _native.check(lib.fg_update_comm(p, B, N, act2.data_ptr(), comm2.data_ptr(), _native.current_stream(DEV)))
                act0 = torch.zeros((B, N, dim_c), device=DEV)
                comm0 = torch.empty((B, N, dim_c), device=DEV)
                _native.check(lib.fg_update_comm_dim(p, B, N, dim_c, act0.data_ptr(), comm0.data_ptr(), _native.current_stream(DEV)))
                torch.cuda.synchronize()
                assert torch.equal(comm0[..., :min(dim_c, 2)], comm2[..., :min(dim_c, 2)]), "pair 0 at dim_c = %d" % dim_c
    print("counter_rng measured: comm noise %.3f of its bound" % used)
