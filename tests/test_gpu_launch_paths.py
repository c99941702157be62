"""GPU parity of every launch path `fg_rollout_hd` can take, at the sizes they are used:

* exactly the launches bench.py times - (27 x 4096, K=20), (9 x 4096, K=20), (81 x 2048, K=20), (243 x 8192, K=4):
  full grids, full LDS residency, the double-buffer wrap over 20 steps, device auto-reset at mixed episode
  phases - against K `env.step` calls bit for bit, plus the fp64 oracle teacher-forced from the GPU's own state
  on a 32-env sample at the first and the last step of the launch;
* World options (walls, max_speed, accel): a rollout launch must integrate the same physics as `env.step`
  (they exist only in step_kernel's options instantiation, which then runs the K-loop);
* agent counts without a specialised kernel (run-time N) through the K-loop, with auto-reset.
"""
import numpy as np
import pytest
import torch

from oracle import formation_oracle as O

pytestmark = pytest.mark.gpu

ATOL = 1e-5


def _make(N, B):
    import formation_gym
    return formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device="cuda:0")


def _np(t):
    return t.detach().double().cpu().numpy()


def _single(N, B, seed, crowd, step0):
    e = _make(N, B)
    e.scenario.seed(seed)
    e.scenario.reset_device(e.world, rng_offset=12345)
    e.world.pos_x.mul_(crowd); e.world.pos_y.mul_(crowd)
    e.world.step_count.copy_(torch.as_tensor(step0, dtype=torch.int32))
    e.auto_reset = True
    return e


def _pair(N, B, seed, crowd, step0):
    """Two envs in the same (device-drawn, crowded) state with mixed episode phases."""
    a, b = _single(N, B, seed, crowd, step0), _single(N, B, seed, crowd, step0)
    for x, y in zip(a.world.get_state() + (a.scenario.ideal_shape,), b.world.get_state() + (b.scenario.ideal_shape,)):
        assert torch.equal(x, y)
    return a, b


def _oracle_step(state, act, sample):
    """fp64 oracle on the sampled envs of a GPU state snapshot."""
    sub = dict(pos=_np(state["pos"][sample]), vel=_np(state["vel"][sample]),
               ideal_shape=_np(state["shape"][sample]), ideal_vel=_np(state["ivel"][sample]),
               step=state["step"][sample].cpu().numpy().astype(np.int32))
    return O.step_hd(sub, _np(act[sample]))


def _snapshot(env):
    pos, vel = env.world.get_state()
    return dict(pos=pos.clone(), vel=vel.clone(), shape=env.scenario.ideal_shape.clone(),
                ivel=env.scenario.ideal_vel.clone(), step=env.world.step_count.clone())


@pytest.mark.parametrize("N,B,K", [(27, 4096, 20), (9, 4096, 20), (81, 2048, 20), (243, 8192, 4),
                                    (9, 5003, 7), (9, 8200, 6), (9, 32768, 4), (27, 16384, 3), (27, 4099, 7), (27, 4099, 3),
                                    (3, 66001, 3), (3, 98400, 20), (4, 114700, 10),   # (the last two: four producer waves per workgroup, a ragged last one)
                                    # agent counts of the other hierarchies (per_layer 2, 4, 5, 8): compile-time-N single steps with
                                    # the rows writer, pipelined rollouts in every batch-size class of launch_roll_* / launch_wide
                                    (4, 5000, 4), (8, 3000, 5), (8, 5000, 4), (16, 8192, 8), (16, 4100, 5), (16, 700, 6), (25, 4096, 20), (25, 600, 5),
                                    (4, 40000, 3), (3, 33000, 5),          # 3 / 4 agents from 32768 envs: one env per lane (fg_hd_lane_kernel.hpp)
                                    # 9 and 8 agents, one workgroup per CU, rollout buffer beyond the Infinity Cache: eight writer waves
                                    (9, 4096, 64), (9, 3000, 70), (8, 4096, 70), (8, 4100, 70), (9, 2048, 110), (9, 1500, 150),
                                    (32, 2048, 20), (32, 16400, 2), (64, 2048, 4), (64, 1000, 3), (125, 600, 3), (125, 40, 3)])
def test_bench_launches_equal_single_steps_and_oracle(N, B, K):
    # the last seven: the batch-size classes that select other instantiations (3 agents: 32-env workgroups from 65 536 envs;
    # 9 agents: 8- and 16-env workgroups with
    # the LDS-tile writer above 4096 envs; 27 agents: the plain tile writer from 16 384 envs and for buffers that fit
    # the Infinity Cache, the HBM-streaming one otherwise) and batches that are not a multiple of the workgroup's env
    # count (a partial last workgroup, step slots that do not start on a 128-byte line)
    rs = np.random.RandomState(N)
    # episode phases: a third of the envs ends its episode inside the launch (at different steps), the rest does not
    Kc = min(K, 99)                                         # launches longer than an episode: every env resets inside
    step0 = np.where(np.arange(B) % 3 == 0, 100 - 1 - (np.arange(B) // 3) % Kc, rs.randint(0, 100 - Kc, B))
    a, b = _pair(N, B, seed=3, crowd=0.45, step0=step0)
    gen = torch.Generator(device="cuda"); gen.manual_seed(N)
    acts = (torch.rand((K, B, N, 2), generator=gen, device="cuda") * 2 - 1).contiguous()
    obs, rew, done, info = b.rollout(acts)                  # no buffers passed: the env's own, placed when beyond the Infinity Cache
    if (N, B, K) == (27, 4096, 20):
        # the launch bench.py times: a placed buffer, hence the 8-writer-wave streaming instantiation
        # rollout_kernel<27,32,512,512,16,10,0,true> - compared with the oracle directly below
        from formation_gym import placement
        assert b.placement["probed"] and b.placement["stages"][0]["arena_GB"] <= 13.0
        if b.placement["kept"] != "as created":
            assert placement.is_placed(obs.data_ptr()) and b.scenario.params(b.world, obs=obs).obs_placed == 1
    sample = torch.as_tensor(rs.choice(B, min(B, 32), replace=False)).cuda()
    n_done = 0
    for k in range(K):
        before = _snapshot(a) if k in (0, K - 1) else None
        o, r, d, i = a.step(acts[k])
        assert torch.equal(o, obs[k]), "observations differ at step %d" % k
        assert torch.equal(r, rew[k]) and torch.equal(d, done[k])
        assert torch.equal(i["individual_reward"], info["individual_reward"][k])
        n_done += int(d[:, 0].sum())
        if before is not None:
            new, out = _oracle_step(before, acts[k], sample)
            np.testing.assert_array_equal(d[sample].cpu().numpy(), out["done"])          # bit-exact
            live = ~out["done"][:, 0]                                                     # envs the launch did not re-draw
            pos, vel = a.world.get_state()
            np.testing.assert_allclose(_np(pos[sample])[live], new["pos"][live], rtol=0, atol=ATOL)
            np.testing.assert_allclose(_np(o[sample])[live], out["obs"][live], rtol=0, atol=ATOL)
            ok = out["cnt_margin"] > 1e-5
            np.testing.assert_allclose(_np(i["individual_reward"][sample])[ok], out["indiv"][ok], rtol=0, atol=ATOL)
            np.testing.assert_allclose(_np(r[sample])[ok, :, 0], out["reward"][ok][..., 0], rtol=2e-6, atol=ATOL)
    if K < 100:
        assert B // 3 - 2 <= n_done <= B // 3 + 2                                           # those episodes really ended inside
    else:
        assert n_done >= B                                                                  # every episode did
    for x, y in zip(a.world.get_state(), b.world.get_state()):
        assert torch.equal(x, y)
    assert torch.equal(a.world.step_count, b.world.step_count)
    assert torch.equal(a.scenario.ideal_shape, b.scenario.ideal_shape) and torch.equal(a.scenario.ideal_vel, b.scenario.ideal_vel)
    assert torch.isfinite(obs).all()
    # the K-step launch's OWN outputs against the oracle, teacher-forced from its start state: step 0 of a fresh launch
    del obs, rew, done, info, o, r, d, i
    b.close(); del b, a
    import gc
    gc.collect(); torch.cuda.empty_cache()
    c = _single(N, B, seed=3, crowd=0.45, step0=step0)
    start = _snapshot(c)
    obs_c, rew_c, done_c, info_c = c.rollout(acts)
    new, out = _oracle_step(start, acts[0], sample)
    np.testing.assert_array_equal(done_c[0][sample].cpu().numpy(), out["done"])
    live = ~out["done"][:, 0]
    np.testing.assert_allclose(_np(obs_c[0][sample])[live], out["obs"][live], rtol=0, atol=ATOL)
    ok = out["cnt_margin"] > 1e-5
    np.testing.assert_allclose(_np(info_c["individual_reward"][0][sample])[ok], out["indiv"][ok], rtol=0, atol=ATOL)


@pytest.mark.parametrize("N,B,K,opts", [(9, 50, 6, dict(max_speed=0.6, accel=3.0, walls=True)),
                                         (27, 37, 5, dict(walls=True)),
                                         (27, 21, 4, dict(max_speed=0.4)),
                                         (81, 5, 3, dict(accel=2.0, walls=True)),
                                         (243, 2, 3, dict(max_speed=0.5))])
def test_rollout_with_world_options_equals_single_steps(N, B, K, opts):
    """env.rollout on a World with walls / max_speed / accel == K env.step calls, bit for bit, and the options are
    really in force (the same rollout without them gives a different trajectory)."""
    from formation_gym.core import Wall
    rs = np.random.RandomState(31 + N)
    st = O.reset_hd(rs.randint(0, 10000, B), N)
    st["pos"] *= 0.9
    acts = torch.as_tensor(rs.uniform(-1, 1, (K, B, N, 2)).astype(np.float32)).cuda()
    step0 = np.where(np.arange(B) % 4 == 0, 98, 7)
    envs = []
    for with_opts in (True, True, False):
        e = _make(N, B)
        e.world.set_state(st["pos"], st["vel"])
        e.scenario.set_formation(e.world, st["ideal_shape"], st["ideal_vel"])
        e.world.step_count.copy_(torch.as_tensor(step0, dtype=torch.int32))
        e.scenario.seed(13); e.auto_reset = True
        if with_opts:
            for ag in e.world.agents:
                ag.max_speed = opts.get("max_speed")
                ag.accel = opts.get("accel")
            if opts.get("walls"):
                e.world.walls = [Wall(o, ax, ep, w) for (o, ax, ep, w) in O.GOLDEN_WALLS]
        envs.append(e)
    a, b, plain = envs
    obs, rew, done, info = b.rollout(acts)
    for k in range(K):
        o, r, d, i = a.step(acts[k])
        assert torch.equal(o, obs[k]) and torch.equal(r, rew[k]) and torch.equal(d, done[k])
        assert torch.equal(i["individual_reward"], info["individual_reward"][k])
    for x, y in zip(a.world.get_state(), b.world.get_state()):
        assert torch.equal(x, y)
    obs_plain = plain.rollout(acts)[0]
    assert not torch.equal(obs_plain[K - 1], obs[K - 1])
    # first step against the fp64 oracle with the same options
    new, out = O.step_hd(dict(pos=np.asarray(st["pos"], np.float32).astype(np.float64), vel=st["vel"],
                              ideal_shape=np.asarray(st["ideal_shape"], np.float32).astype(np.float64),
                              ideal_vel=np.asarray(st["ideal_vel"], np.float32).astype(np.float64),
                              step=step0.astype(np.int32)), _np(acts[0]),
                         max_speed=opts.get("max_speed"), accel=opts.get("accel"),
                         walls=O.GOLDEN_WALLS if opts.get("walls") else None)
    live = ~out["done"][:, 0]
    np.testing.assert_allclose(_np(obs[0])[live], out["obs"][live], rtol=0, atol=ATOL)


@pytest.mark.parametrize("N,B,K", [(10, 41, 7), (33, 9, 5), (100, 3, 4), (300, 2, 3)])
def test_rollout_with_runtime_agent_count_equals_single_steps(N, B, K):
    """Agent counts without a specialised kernel: the K-loop of the run-time-N step kernel, device auto-reset on."""
    rs = np.random.RandomState(N)
    step0 = np.where(np.arange(B) % 2 == 0, 100 - 2, 11)
    a, b = _pair(N, B, seed=8, crowd=0.4, step0=step0)
    acts = torch.as_tensor(rs.uniform(-1, 1, (K, B, N, 2)).astype(np.float32)).cuda()
    obs, rew, done, info = b.rollout(acts)
    for k in range(K):
        o, r, d, i = a.step(acts[k])
        assert torch.equal(o, obs[k]) and torch.equal(r, rew[k]) and torch.equal(d, done[k])
    assert done.any() and not done.all()
    for x, y in zip(a.world.get_state(), b.world.get_state()):
        assert torch.equal(x, y)
    assert torch.equal(a.scenario.ideal_shape, b.scenario.ideal_shape)


def _strided_obs(shape_prefix, N, pitch, fill):
    """Observation tensor [.., B, N, 6N] whose env blocks are `pitch` floats apart, pad pre-filled with `fill`."""
    buf = torch.full(tuple(shape_prefix) + (pitch,), fill, device="cuda")
    return buf, buf[..., :6 * N * N].view(tuple(shape_prefix) + (N, 6 * N))


@pytest.mark.parametrize("N,B,K", [(27, 70, 5), (9, 130, 6), (3, 40, 4), (81, 7, 4), (243, 5, 3), (10, 33, 4), (100, 3, 3),
                                    (27, 4100, 8),           # large enough for the HBM-streaming tile writer
                                    (9, 5000, 4), (8, 4100, 4)])   # the gather writer (8 agents: a pitch of an odd number of 8-byte
                                                                   # units, so that env blocks alternate between the two 16-byte phases)
def test_padded_observation_env_pitch(N, B, K):
    """FgParams.obs_env_pitch: env blocks on their own 128-byte lines (a strided [B, N, 6N] view).  Every entry point
    that writes observations gives the bits of the contiguous layout, the pad is left alone (rollout launches may
    zero-fill it up to the env's last 128-byte line), and the controller reads the strided rows."""
    from formation_gym.policy_bfs import bfs_actions
    pitch = 6 * N * N + 2 if N == 8 else -(-6 * N * N // 32) * 32 + (32 if N == 9 else 0)
    rs = np.random.RandomState(N)
    step0 = np.where(np.arange(B) % 2 == 0, 100 - 2, 9)
    a, b = _pair(N, B, seed=4, crowd=0.5, step0=step0)
    acts = torch.as_tensor(rs.uniform(-1, 1, (K, B, N, 2)).astype(np.float32)).cuda()
    # reset observation (fg_observe_hd)
    buf, view = _strided_obs((B,), N, pitch, -7.0)
    b.scenario.observe_batch(b.world, {"obs": view, "reward": b._out["reward"]})
    a.scenario.observe_batch(a.world, {"obs": a._out["obs"], "reward": a._out["reward"]})
    assert torch.equal(view, a._out["obs"]) and (buf[:, 6 * N * N:] == -7.0).all()
    if N in (27, 9, 3, 81, 243):
        assert torch.equal(bfs_actions(view, 3), bfs_actions(a._out["obs"], 3))
    # single step (fg_step_hd) into a strided buffer
    buf1, view1 = _strided_obs((B,), N, pitch, -7.0)
    out1 = dict(b._out, obs=view1)
    b.scenario.step_batch(b.world, acts[0], out1, auto_reset=True, rng_offset=1)
    a.scenario.step_batch(a.world, acts[0], a._out, auto_reset=True, rng_offset=1)
    assert torch.equal(view1, a._out["obs"]) and torch.equal(out1["reward"], a._out["reward"])
    assert (buf1[:, 6 * N * N:] == -7.0).all()
    # K-step launch (fg_rollout_hd) into a strided rollout buffer
    bufk, viewk = _strided_obs((K - 1, B), N, pitch, -7.0)
    outk = dict(obs=viewk, reward=torch.empty((K - 1, B, N), device="cuda"), indiv=torch.empty((K - 1, B, N), device="cuda"),
                done=torch.zeros((K - 1, B, N), dtype=torch.uint8, device="cuda"))
    b.scenario.rollout_batch(b.world, acts[1:], outk, auto_reset=True, rng_offset=2)
    for k in range(1, K):
        a.scenario.step_batch(a.world, acts[k], a._out, auto_reset=True, rng_offset=1 + k)
        assert torch.equal(viewk[k - 1], a._out["obs"]) and torch.equal(outk["reward"][k - 1], a._out["reward"])
    padk = bufk[..., 6 * N * N:]                       # untouched, or zero-filled up to the env's last cache line
    assert ((padk == -7.0) | (padk == 0.0)).all()      # (the LDS-tile writer completes that line: fg_obs_writers.hpp)
    for x, y in zip(a.world.get_state(), b.world.get_state()):
        assert torch.equal(x, y)
    # a pitch the kernels cannot take is refused
    from formation_gym import _native
    bad = torch.empty((B, 6 * N * N + 1), device="cuda")[:, :6 * N * N].view(B, N, 6 * N)
    with pytest.raises(ValueError):
        b.scenario.observe_batch(b.world, {"obs": bad, "reward": b._out["reward"]})
    p = b.scenario.params(b.world)
    p.obs_env_pitch = 6 * N * N - 2
    assert _native.load().fg_observe_hd(p, B, N, *([b.world.pos_x.data_ptr()] * 7), view.data_ptr(), *([None] * 7)) \
        == _native.FG_ERR_BAD_ARG


@pytest.mark.parametrize("N,B", [(27, 256), (9, 1000), (81, 64), (16, 100)])
def test_step_loop_can_be_captured_in_a_hip_graph(N, B):
    """A caller with a device-side policy between the steps (here a fixed linear map of the observation, torch ops)
    can capture the whole loop - policy, fg_step_hd, the built-in controller fg_policy_bfs - in a hipGraph and replay
    it: the library only enqueues kernels on the caller's stream (no allocation, no synchronisation, no host read-back).
    The replay must give what the same loop gives launch by launch.  Auto-reset is off inside the graph: `rng_offset`
    is a by-value launch argument, so a replayed graph would repeat its reset draws."""
    import formation_gym
    T = 6
    dev = "cuda:0"
    gen = torch.Generator(device=dev); gen.manual_seed(N)
    W = (torch.rand((6 * N, 2), generator=gen, device=dev) - 0.5) * 0.2
    per = 3 if N in (9, 27, 81) else 4

    def loop(env, obs, rec):
        for t in range(T):
            act = torch.tanh(obs @ W) if t % 2 == 0 else formation_gym.get_action_BFS(formation_gym.ezpolicy, obs, per)
            obs, rew, done, info = env.step(act.contiguous())
            rec["obs"][t].copy_(obs); rec["rew"][t].copy_(rew); rec["ind"][t].copy_(info["individual_reward"])

    def fresh():
        env = _make(N, B)
        env.seed(4); env.reset()
        env.auto_reset = False
        rec = dict(obs=torch.zeros((T, B, N, 6 * N), device=dev), rew=torch.zeros((T, B, N, 1), device=dev),
                   ind=torch.zeros((T, B, N), device=dev))
        return env, rec

    eager, rec_e = fresh()
    loop(eager, eager._out["obs"], rec_e)

    env, rec_g = fresh()
    state0 = [x.clone() for x in env.world.get_state()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # warm-up on the capture stream (binds launchers, raises LDS limits)
        loop(env, env._out["obs"], rec_g)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        loop(env, env._out["obs"], rec_g)
    for replay in range(2):                               # the state the graph starts from is restored by the caller
        env.world.set_state(*state0)
        env.world.step_count.zero_()
        env.scenario.observe_batch(env.world, env._out)
        for v in rec_g.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in rec_e:
            assert torch.equal(rec_e[k], rec_g[k]), "graph replay %d differs from the launch-by-launch loop in %s" % (replay, k)
    for x, y in zip(eager.world.get_state(), env.world.get_state()):
        assert torch.equal(x, y)


@pytest.mark.parametrize("N,B", [(27, 300), (9, 64)])
def test_captured_loop_with_auto_reset_uses_the_device_rng_counter(N, B):
    """Auto-reset inside a replayed hipGraph: the per-step offset of the counter RNG is read from device memory
    (FgParams.rng_offset_dev) and advanced by a device-side add the graph contains, so every replay draws NEW reset
    states - exactly those of the same number of steps taken launch by launch (with or without the device counter)."""
    T, R = 5, 3                                           # steps per graph, replays
    dev = "cuda:0"
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    acts = torch.rand((T, B, N, 2), generator=gen, device=dev) * 2 - 1

    def fresh(counter):
        env = _make(N, B)
        env.seed(9); env.reset()
        env.auto_reset = True
        env.world.world_length = 3                         # short episodes: every env restarts in every replay
        env.world.step_count.copy_(torch.arange(B, dtype=torch.int32, device=dev) % 3)
        if counter:
            env.use_device_rng_counter()
        return env

    def loop(env, rec, base):
        for t in range(T):
            obs, rew, done, info = env.step(acts[t])
            rec["obs"][base + t].copy_(obs); rec["done"][base + t].copy_(done)

    def rec():
        return dict(obs=torch.zeros((T * (R + 1), B, N, 6 * N), device=dev), done=torch.zeros((T * (R + 1), B, N), dtype=torch.bool, device=dev))

    plain, rec_p = fresh(False), rec()                    # by-value offsets, launch by launch
    for r in range(R + 1):
        loop(plain, rec_p, r * T)
    eager, rec_e = fresh(True), rec()                     # device counter, launch by launch
    for r in range(R + 1):
        loop(eager, rec_e, r * T)
    assert torch.equal(rec_p["obs"], rec_e["obs"]) and torch.equal(rec_p["done"], rec_e["done"])
    assert int(eager.world.rng_counter.item()) == T * (R + 1)

    env, rec_g = fresh(True), rec()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # warm-up on the capture stream = the first T steps
        loop(env, rec_g, 0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    scratch = rec()
    graph = torch.cuda.CUDAGraph()
    state = [x.clone() for x in (env.world.pos_x, env.world.pos_y, env.world.vel_x, env.world.vel_y, env.world.step_count,
                                 env.scenario.ideal_shape, env.scenario.ideal_vel, env.world.rng_counter)]
    with torch.cuda.graph(graph, stream=side):
        loop(env, scratch, 0)
    for dst, src in zip((env.world.pos_x, env.world.pos_y, env.world.vel_x, env.world.vel_y, env.world.step_count,
                         env.scenario.ideal_shape, env.scenario.ideal_vel, env.world.rng_counter), state):
        dst.copy_(src)                                    # capture does not execute, but be explicit about the start state
    for r in range(1, R + 1):
        graph.replay()
        torch.cuda.synchronize()
        rec_g["obs"][r * T:(r + 1) * T].copy_(scratch["obs"][:T]); rec_g["done"][r * T:(r + 1) * T].copy_(scratch["done"][:T])
    assert torch.equal(rec_g["done"], rec_p["done"])
    assert torch.equal(rec_g["obs"], rec_p["obs"])
    for r in range(R + 1):                                               # every env restarted in every block of T steps,
        assert bool(rec_p["done"][r * T:(r + 1) * T, :, 0].any(0).all())
    blocks = rec_p["obs"].view(R + 1, T, B, N, 6 * N)
    assert not torch.equal(blocks[1], blocks[2])                         # ... with different draws from block to block
    assert int(env.world.rng_counter.item()) == T * (R + 1)


@pytest.mark.parametrize("scenario,kind,N,B", [("formation_hd_partial_env", "partial", 70, 9), ("formation_hd_partial_range_env", "range", 130, 5),
                                                ("formation_hd_obs_env", "obstacle", 100, 6), ("formation_hd_obs_env", "obstacle", 62, 7),
                                                ("formation_hd_partial_env", "partial", 300, 2), ("basic_formation_env", "basic", 90, 5)])
def test_landmark_scenarios_beyond_64_entities(scenario, kind, N, B):
    """fg_step_scenario / fg_step_basic with more than 64 movable entities (one env per workgroup instead of per lane
    group of a wave; 62 agents + 3 obstacles crosses the limit through the obstacles) against the fp64 oracle on the same
    crowded fp32 state, three steps teacher-forced."""
    import formation_gym
    rs = np.random.RandomState(N)
    env = formation_gym.make_env(scenario, False, N, num_envs=B, device="cuda:0")
    P = O.BasicParams() if kind == "basic" else O.ScnParams(kind)
    L, M = P.num_landmarks, getattr(P, "num_obstacles", 0)
    f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
    state = dict(pos=f32(rs.uniform(-1, 1, (B, N, 2)) * 0.8), vel=f32(rs.uniform(-0.3, 0.3, (B, N, 2))),
                 landmarks=f32(rs.uniform(-1, 1, (B, L, 2))), step=np.zeros(B, dtype=np.int32))
    if M:
        state["obst_pos"] = f32(rs.uniform(-0.5, 0.5, (B, M, 2)))
        state["obst_vel"] = f32(np.tile(np.array(P.obstacle_vel), (B, M, 1)))
    elif kind != "basic":
        state["obst_pos"] = np.zeros((B, 0, 2)); state["obst_vel"] = np.zeros((B, 0, 2))
    for t in range(3):
        env.world.set_state(state["pos"], state["vel"])
        env.world.landmark_pos.copy_(torch.as_tensor(state["landmarks"], dtype=torch.float32))
        if M:
            env.world.obstacle_pos.copy_(torch.as_tensor(state["obst_pos"], dtype=torch.float32))
            env.world.obstacle_vel.copy_(torch.as_tensor(state["obst_vel"], dtype=torch.float32))
        env.world.step_count.fill_(t)
        act = f32(rs.uniform(-1, 1, (B, N, 2)))
        obs, rew, done, info = env.step(torch.as_tensor(act, dtype=torch.float32).cuda())
        new, out = (O.step_basic(state, act, P) if kind == "basic" else O.step_scn(kind, state, act, P))
        pos, vel = env.world.get_state()
        np.testing.assert_allclose(_np(pos), new["pos"], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(vel), new["vel"], rtol=0, atol=ATOL)
        np.testing.assert_allclose(_np(obs), out["obs"], rtol=0, atol=ATOL)
        if M:
            np.testing.assert_allclose(_np(env.world.obstacle_pos), new["obst_pos"], rtol=0, atol=ATOL)
            np.testing.assert_allclose(_np(env.world.obstacle_vel), new["obst_vel"], rtol=0, atol=ATOL)
        # collision counts are integers: compare where no pair sits within 1e-5 of a threshold
        PD = np.sqrt(((new["pos"][:, :, None] - new["pos"][:, None]) ** 2).sum(-1)) + (0 if kind == "basic" else 10 * np.eye(N))
        ok = np.abs(PD - P.collide_thresh).min((1, 2)) > 1e-5
        if M:
            OD = np.sqrt(((new["pos"][:, :, None] - new["obst_pos"][:, None]) ** 2).sum(-1))
            ok &= np.abs(OD - (P.agent_size + P.obstacle_size)).min((1, 2)) > 1e-5
        assert ok.sum() >= B - 2
        np.testing.assert_allclose(_np(info["individual_reward"])[ok], out["indiv"][ok], rtol=0, atol=2 * ATOL)   # |r| up to ~20 at these counts
        np.testing.assert_allclose(_np(rew)[ok][..., 0], np.repeat(out["shared"][:, None], N, 1)[ok], rtol=2e-6, atol=ATOL)
        np.testing.assert_array_equal(done.cpu().numpy(), out["done"])
        state = dict(new, pos=f32(new["pos"]), vel=f32(new["vel"]))
        if M:
            state["obst_pos"] = f32(new["obst_pos"]); state["obst_vel"] = f32(new["obst_vel"])


@pytest.mark.parametrize("N,B_split", [(243, 96), (100, 128), (81, 128), (300, 128), (1024, 5)])
def test_split_step_equals_the_fused_launch(N, B_split):
    """More than 64 agents and few envs: `fg_step_hd` runs the fused kernel without the observation and a second launch in
    which several workgroups per env stream the observation (launch_step in formation_hip.hip).  The same envs stepped in a
    batch one env larger - which takes the single fused launch - must give the same bits, auto-reset included."""
    B = B_split + 1
    if N == 1024:
        B = 130                                            # the fused launch needs more than 128 envs
    step0 = np.where(np.arange(B) % 3 == 0, 99, 5)
    big, _ = _pair(N, B, seed=6, crowd=0.4, step0=step0)
    small = _make(N, B_split)
    small.scenario.seed(6)
    pos, vel = big.world.get_state()
    small.world.set_state(pos[:B_split], vel[:B_split])
    small.scenario.ideal_shape.copy_(big.scenario.ideal_shape[:B_split]); small.scenario.ideal_vel.copy_(big.scenario.ideal_vel[:B_split])
    small.world.step_count.copy_(big.world.step_count[:B_split])
    small.auto_reset = True
    gen = torch.Generator(device="cuda"); gen.manual_seed(N)
    for t in range(3):
        act = torch.rand((B, N, 2), generator=gen, device="cuda") * 2 - 1
        o1, r1, d1, i1 = big.step(act)
        o2, r2, d2, i2 = small.step(act[:B_split].contiguous())
        assert torch.equal(o1[:B_split], o2) and torch.equal(r1[:B_split], r2) and torch.equal(d1[:B_split], d2)
        assert torch.equal(i1["individual_reward"][:B_split], i2["individual_reward"])
        assert bool(d2.any()) == (t == 0)
    for x, y in zip(big.world.get_state(), small.world.get_state()):
        assert torch.equal(x[:B_split], y)
    assert torch.equal(big.scenario.ideal_shape[:B_split], small.scenario.ideal_shape)


def test_device_rng_counter_toggle_and_captured_rollouts():
    """(1) Switching the device RNG counter on and off in the middle of a run changes nothing: the offsets continue.
    (2) K-step launches (`env.rollout`, `env.rollout_policy` into caller-owned buffers) are capturable too: a graph of
    two launches replayed three times equals the same launches issued one by one."""
    N, B, K = 27, 200, 6
    dev = "cuda:0"
    gen = torch.Generator(device=dev); gen.manual_seed(3)
    acts = torch.rand((K, B, N, 2), generator=gen, device=dev) * 2 - 1

    def fresh():
        env = _make(N, B)
        env.seed(2); env.reset()
        env.auto_reset = True
        env.world.world_length = 4
        env.world.step_count.copy_(torch.arange(B, dtype=torch.int32, device=dev) % 4)
        return env

    def bufs():
        f = dict(dtype=torch.float32, device=dev)
        return dict(obs=torch.empty((K, B, N, 6 * N), **f), reward=torch.empty((K, B, N), **f), indiv=torch.empty((K, B, N), **f),
                    done=torch.zeros((K, B, N), dtype=torch.uint8, device=dev), act=torch.empty((K, B, N, 2), **f))

    # (1) toggle
    a, b = fresh(), fresh()
    seq_a, seq_b = [], []
    for t in range(9):
        if t == 2:
            b.use_device_rng_counter(True)
        if t == 6:
            b.use_device_rng_counter(False)
        seq_a.append(a.step(acts[t % K])[0].clone()); seq_b.append(b.step(acts[t % K])[0].clone())
    assert all(torch.equal(x, y) for x, y in zip(seq_a, seq_b))
    assert b.world.rng_counter is None and a._rng_offset == b._rng_offset == 9

    # (2) captured K-step launches
    ref, out_r, pol_r = fresh(), bufs(), bufs()
    rec = []
    for r in range(4):
        ref.rollout(acts, out={k: v for k, v in out_r.items() if k != "act"})
        ref.rollout_policy(K, 3, out=pol_r)
        rec.append((out_r["obs"].clone(), pol_r["obs"].clone(), pol_r["act"].clone()))
    env, out_g, pol_g = fresh(), bufs(), bufs()
    env.use_device_rng_counter()
    out_g_roll = {k: v for k, v in out_g.items() if k != "act"}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                        # = block 0, launch by launch
        env.rollout(acts, out=out_g_roll)
        env.rollout_policy(K, 3, out=pol_g)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(out_g["obs"], rec[0][0]) and torch.equal(pol_g["obs"], rec[0][1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        env.rollout(acts, out=out_g_roll)
        env.rollout_policy(K, 3, out=pol_g)
    for r in range(1, 4):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out_g["obs"], rec[r][0]), "replay %d: open-loop launch" % r
        assert torch.equal(pol_g["obs"], rec[r][1]) and torch.equal(pol_g["act"], rec[r][2]), "replay %d: closed-loop launch" % r
    for x, y in zip(ref.world.get_state(), env.world.get_state()):
        assert torch.equal(x, y)


@pytest.mark.parametrize("N,B,policy", [(27, 300, "bfs"), (9, 640, "linear"), (81, 40, "bfs_out")])
def test_vec_env_capture_replays_equal_the_step_loop(N, B, policy):
    """FormationVecEnv.capture(policy_fn, T): three replays of the captured T-step loop (device-side policy + vec-env
    step with auto-resets inside the graph) equal 3 T steps of the same loop taken launch by launch, bit for bit -
    observations, rewards, dones, actions, final state - and capturing leaves the env's state untouched."""
    import formation_gym
    from formation_gym.vec_env import FormationVecEnv
    T, R = 5, 3
    dev = "cuda:0"
    gen = torch.Generator(device=dev); gen.manual_seed(N)
    W = (torch.rand((6 * N, 2), generator=gen, device=dev) - 0.5) * 0.2
    if policy == "bfs":
        fn = lambda obs: formation_gym.get_action_BFS(formation_gym.ezpolicy, obs, 3)
    elif policy == "bfs_out":                              # a policy that writes into the slot it is given
        fn = lambda obs, out=None: formation_gym.get_action_BFS(formation_gym.ezpolicy, obs, 3, out=out)
    else:
        fn = lambda obs: torch.tanh(obs @ W)

    def fresh():
        v = FormationVecEnv(_make(N, B), reset_mode="device")
        v.env.seed(6)
        v.reset()
        v.env.world.world_length = 4                       # short episodes: resets inside every replay
        v.env.world.step_count.copy_(torch.arange(B, dtype=torch.int32, device=dev) % 4)
        return v

    ref = fresh()
    obs = ref.env._out["obs"]
    want = {k: [] for k in ("obs", "rew", "done", "act")}
    for t in range(T * R):
        act = fn(obs).contiguous()
        want["act"].append(act.clone())
        obs, rew, done, info = ref.step(act)
        want["obs"].append(obs.clone()); want["rew"].append(rew.clone()); want["done"].append(done.clone())

    v = fresh()
    before = [x.clone() for x in v.env.world.get_state()] + [v.env.world.step_count.clone()]
    loop = v.capture(fn, T)
    after = [x.clone() for x in v.env.world.get_state()] + [v.env.world.step_count.clone()]
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    for r in range(R):
        o, rw, d, info = loop.replay()
        torch.cuda.synchronize()
        for t in range(T):
            k = r * T + t
            assert torch.equal(o[t], want["obs"][k]), (r, t)
            assert torch.equal(rw[t], want["rew"][k]) and torch.equal(d[t], want["done"][k])
            assert torch.equal(info["actions"][t], want["act"][k])
    for x, y in zip(ref.env.world.get_state(), v.env.world.get_state()):
        assert torch.equal(x, y)
    assert torch.stack(want["done"]).any() and v.env.current_step == ref.env.current_step == T * R
    with pytest.raises(NotImplementedError):
        FormationVecEnv(_make(N, 8), reset_mode="host").capture(fn, 2)


@pytest.mark.parametrize("N,B_split", [(81, 1), (100, 96), (243, 96), (243, 1), (81, 128)])
def test_split_step_with_index_outputs_world_options_and_padded_pitch(N, B_split):
    """The split single step: landmark-index outputs, World options (walls + max_speed: the OPTS instantiation),
    a padded observation pitch and auto-reset at the reset step, each against the same envs inside a batch large enough to
    take the single fused launch - bit for bit."""
    from formation_gym.core import Wall
    B = 140
    step0 = np.where(np.arange(B) % 2 == 0, 99, 7)
    pitch = -(-6 * N * N // 32) * 32 + 32

    def build(nenv, opts):
        e = _make(N, nenv)
        e.scenario.seed(8)
        if opts:
            for a in e.world.agents:
                a.max_speed = 0.7
            e.world.walls = [Wall("V", -0.8, (-1.0, 1.0), 0.1), Wall("H", 0.7, (-0.5, 0.5), 0.2)]
        e.auto_reset = True
        e.enable_assignments(True)
        return e

    for opts in (False, True):
        big = build(B, opts)
        big.scenario.reset_device(big.world, rng_offset=777)
        big.world.pos_x.mul_(0.4); big.world.pos_y.mul_(0.4)
        big.world.step_count.copy_(torch.as_tensor(step0, dtype=torch.int32))
        small = build(B_split, opts)
        pos, vel = big.world.get_state()
        small.world.set_state(pos[:B_split], vel[:B_split])
        small.scenario.ideal_shape.copy_(big.scenario.ideal_shape[:B_split]); small.scenario.ideal_vel.copy_(big.scenario.ideal_vel[:B_split])
        small.world.step_count.copy_(big.world.step_count[:B_split])
        outs = []
        for e, n in ((big, B), (small, B_split)):
            f = dict(dtype=torch.float32, device="cuda")
            raw = torch.full((n, pitch), -7.0, **f)
            out = dict(obs=raw[:, :6 * N * N].view(n, N, 6 * N), reward=torch.empty((n, N), **f), indiv=torch.empty((n, N), **f),
                       done=torch.zeros((n, N), dtype=torch.uint8, device="cuda"),
                       near_lm=torch.zeros((n, N), dtype=torch.int32, device="cuda"),
                       near_ag=torch.zeros((n, N), dtype=torch.int32, device="cuda"),
                       hd_idx=torch.zeros((n, 4), dtype=torch.int32, device="cuda"))
            outs.append((out, raw))
        gen = torch.Generator(device="cuda"); gen.manual_seed(N + B_split)
        for t in range(2):
            act = torch.rand((B, N, 2), generator=gen, device="cuda") * 2 - 1
            big.scenario.step_batch(big.world, act, outs[0][0], auto_reset=True, rng_offset=5 + t)
            small.scenario.step_batch(small.world, act[:B_split].contiguous(), outs[1][0], auto_reset=True, rng_offset=5 + t)
            for k in outs[0][0]:
                assert torch.equal(outs[0][0][k][:B_split], outs[1][0][k]), (opts, t, k)
            assert bool((outs[1][1][:, 6 * N * N:] == -7.0).all())            # the pad between env blocks is untouched
            assert bool(outs[1][0]["done"].any()) == (t == 0)
        for x, y in zip(big.world.get_state(), small.world.get_state()):
            assert torch.equal(x[:B_split], y)
        assert torch.equal(big.scenario.ideal_shape[:B_split], small.scenario.ideal_shape)


@pytest.mark.parametrize("N,B,K", [(27, 4096, 8), (27, 4099, 7), (81, 1024, 4), (243, 512, 2)])
def test_placed_rollout_buffers_equal_step_calls(N, B, K):
    """env.alloc_rollout_buffers: the observation buffer composed of physical chunks spread over the device memory
    (fg_arena_*, formation_gym/placement.py).  A rollout into it - at 27 agents the instantiation with 8 paced writer waves
    that FgParams.obs_placed selects - equals K step calls bit for bit; the probe leaves the env's state untouched."""
    from formation_gym import placement
    rs = np.random.RandomState(N + K)
    step0 = np.where(np.arange(B) % 3 == 0, 100 - 1 - (np.arange(B) // 3) % K, rs.randint(0, 100 - K, B))
    a, b = _pair(N, B, seed=4, crowd=0.45, step0=step0)
    before = [x.clone() for x in b.world.get_state()] + [b.world.step_count.clone(), b.scenario.ideal_shape.clone()]
    out = b.alloc_rollout_buffers(K)
    after = [x.clone() for x in b.world.get_state()] + [b.world.step_count.clone(), b.scenario.ideal_shape.clone()]
    for x, y in zip(before, after):
        assert torch.equal(x, y)
    rep = b.placement
    assert rep["probed"] and rep["tried"] >= 2 and rep["kept_ms"] <= rep["worst_ms"]
    if rep["kept"] != "as created":
        assert placement.is_placed(out["obs"].data_ptr()) and b.scenario.params(b.world, obs=out["obs"]).obs_placed == 1
    assert not placement.is_placed(a._out["obs"].data_ptr())
    gen = torch.Generator(device="cuda"); gen.manual_seed(N)
    acts = (torch.rand((K, B, N, 2), generator=gen, device="cuda") * 2 - 1).contiguous()
    for rep_ in range(2):                                   # two launches into the same placed buffer
        obs, rew, done, info = b.rollout(acts, out=out)
        for k in range(K):
            o, r, d, i = a.step(acts[k])
            assert torch.equal(o, obs[k]), "observations differ at step %d" % k
            assert torch.equal(r, rew[k]) and torch.equal(d, done[k])
            assert torch.equal(i["individual_reward"], info["individual_reward"][k])
    for x, y in zip(a.world.get_state(), b.world.get_state()):
        assert torch.equal(x, y)
    # the single-step buffer, placed
    if N >= 81:
        rep2 = b.place_step_buffers()
        assert rep2["probed"] == (B * N * 6 * N * 4 >= placement.MIN_PROBE_BYTES)      # 81 x 1024: 161 MB, cache-resident
        act = torch.rand((B, N, 2), generator=gen, device="cuda") * 2 - 1
        o1, r1, d1, _ = a.step(act)
        o2, r2, d2, _ = b.step(act)
        assert torch.equal(o1, o2) and torch.equal(r1, r2) and torch.equal(d1, d2)
    del out, obs


def test_placed_closed_loop_rollout_equals_policy_and_step_calls():
    """env.rollout_policy into placed buffers (27 agents: the closed-loop instantiation with 8 writer waves and the rows
    writer that FgParams.obs_placed selects) == K x (get_action_BFS on the last observation, step), bit for bit."""
    import formation_gym
    N, B, K = 27, 4096, 8
    step0 = (np.arange(B) * 5) % 100
    a, b = _pair(N, B, seed=9, crowd=0.6, step0=step0)
    out = b.alloc_rollout_buffers(K, policy=True)
    assert b.placement["probed"]
    for e in (a, b):
        e.scenario.observe_batch(e.world, {"obs": e._out["obs"], "reward": e._out["reward"]})
    start = _snapshot(b)
    obs, rew, done, info = b.rollout_policy(K, 3, out=out)
    # the closed-loop launch's own first step against the oracle (state + the actions the launch recorded)
    sample = torch.arange(0, B, 131, device="cuda")
    new, want = _oracle_step(start, info["actions"][0], sample)
    live = ~want["done"][:, 0]
    np.testing.assert_allclose(_np(obs[0][sample])[live], want["obs"][live], rtol=0, atol=ATOL)
    o = a._out["obs"]
    for k in range(K):
        act = formation_gym.get_action_BFS(formation_gym.ezpolicy, o, 3)
        assert torch.equal(act, info["actions"][k]), k
        o, r, d, i = a.step(act)
        assert torch.equal(o, obs[k]) and torch.equal(r, rew[k]) and torch.equal(d, done[k])
    for x, y in zip(a.world.get_state(), b.world.get_state()):
        assert torch.equal(x, y)
    assert bool(done.any())


def test_arena_mappings_get_fresh_addresses_and_chunks_keep_their_contents():
    """The discipline of fg_arena_* (include/formation_hip.h): a chunk has one address at a time, an address range that
    held a mapping is never handed out again (on this stack a mapping at a reused address corrupts the chunks mapped
    there before: profiles/r03_place/va_reuse_check.txt), chunks keep their contents across unmap / map, and trimmed
    memory goes back to the driver."""
    from formation_gym import _native, placement
    dev = torch.device("cuda:0")
    CH, W = 32 << 20, 4

    def free_bytes():                                       # without what torch's own allocator caches
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        return torch.cuda.mem_get_info(dev)[0]

    x = torch.zeros(1 << 20, device=dev); x.fill_(1.0)     # the kernels used below, loaded before memory is counted
    assert bool((x == 1.0).all()) and float(x.sum()) == float(1 << 20)
    del x
    free0 = free_bytes()
    retired0 = _native.load().fg_arena_retired_address_bytes()
    arena = placement.Arena(4 * W * CH, dev, CH)
    assert arena.chunks == 4 * W and arena.chunk == CH
    assert _native.load().fg_arena_retired_address_bytes() >= retired0 + 4 * W * CH      # the placing pass at creation
    nfl = W * CH // 4
    seen = []
    for r in range(4):
        A = list(range(0, 2 * W, 2)) if r % 2 == 0 else list(range(2 * W, 4 * W, 2))    # spread selections
        Bc = [c + 1 for c in A]
        va = arena.map(A)
        with pytest.raises(_native.FormationHipError):                                  # a mapped chunk cannot be mapped again
            arena.map([A[0], Bc[1], Bc[2], Bc[3]])
        ta = arena.floats(va, nfl); ta.fill_(float(r + 1)); torch.cuda.synchronize(); del ta
        arena.unmap(va)
        vb = arena.map(Bc)
        tb = arena.floats(vb, nfl); tb.fill_(-float(r + 1)); torch.cuda.synchronize()
        assert bool((tb == -float(r + 1)).all())
        del tb
        arena.unmap(vb)
        va2 = arena.map(A)
        ta = arena.floats(va2, nfl)
        assert bool((ta == float(r + 1)).all()), "chunks lost their contents across unmap / map (round %d)" % r
        del ta
        arena.unmap(va2)
        seen += [va, vb, va2]
    spans = sorted((v, v + W * CH) for v in seen)
    assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:])), "an address range was handed out twice"
    keep = arena.map([1, 5, 9, 13])
    arena.trim()
    assert free0 - free_bytes() < W * CH + (128 << 20)                                  # everything but the kept chunks is back
    with pytest.raises(_native.FormationHipError):
        arena.map([0, 2, 4, 6])                                                         # trimmed chunks are gone
    t = arena.floats(keep, nfl); t.fill_(3.0); torch.cuda.synchronize()
    assert float(t.sum()) == 3.0 * nfl
    del t
    arena.close()
    assert free0 - free_bytes() < (128 << 20)


@pytest.mark.parametrize("N,B,K,obs_every,pad", [(27, 4096, 8, 2, False), (27, 4096, 6, 1, True), (81, 1024, 4, 2, True),
                                                 # 9 / 8 agents: the span form of the gather writer with every 2nd observation kept,
                                                 # and a padded env pitch (the per-env form)
                                                 # (9 x 8192 and up into a buffer beyond the Infinity Cache: 32-env workgroups;
                                                 # 49169 envs: a ragged last workgroup among 1537)
                                                 (9, 8192, 60, 2, False), (9, 8192, 26, 1, True), (9, 49169, 6, 1, False), (9, 14350, 12, 1, False),
                                                 # 8 / 16 agents beyond the Infinity Cache: 32-env workgroups / eight writer waves
                                                 (8, 12300, 50, 1, False), (8, 16384, 40, 2, False), (16, 8200, 17, 1, False)])
def test_placed_rollout_buffers_with_obs_every_and_env_pitch(N, B, K, obs_every, pad):
    """alloc_rollout_buffers with every obs_every-th observation kept and / or env blocks padded to whole 128-byte lines
    (FgParams.obs_env_pitch): the placed, strided buffer takes the same bits as K step calls."""
    a, b = _pair(N, B, seed=6, crowd=0.4, step0=(np.arange(B) * 3) % 100)
    pitch = -(-6 * N * N // 32) * 32 if pad else 0
    out = b.alloc_rollout_buffers(K, obs_every=obs_every, obs_env_pitch=pitch)
    assert b.placement["probed"]
    assert tuple(out["obs"].shape) == (K // obs_every, B, N, 6 * N)
    if pad:
        assert out["obs"].stride(1) == pitch and not out["obs"].is_contiguous()
    gen = torch.Generator(device="cuda"); gen.manual_seed(N + K)
    acts = (torch.rand((K, B, N, 2), generator=gen, device="cuda") * 2 - 1).contiguous()
    obs, rew, done, info = b.rollout(acts, out=out, obs_every=obs_every)
    for k in range(K):
        o, r, d, i = a.step(acts[k])
        assert torch.equal(r, rew[k]) and torch.equal(d, done[k])
        if (k + 1) % obs_every == 0:
            assert torch.equal(o, obs[k // obs_every]), "observations differ at step %d" % k
    for x, y in zip(a.world.get_state(), b.world.get_state()):
        assert torch.equal(x, y)


@pytest.mark.parametrize("N,B,K", [(27, 300, 6), (27, 513, 6), (27, 1024, 5), (27, 1031, 5), (27, 2048, 4), (27, 2049, 4),
                                   (27, 2048, 20), (27, 2563, 12), (243, 200, 3), (243, 520, 2), (81, 512, 4), (81, 520, 4)])
def test_small_batch_rollout_geometries_equal_step_calls(N, B, K):
    """Rollout launches of batches that do not fill the chip take workgroups of fewer envs (27 agents: 2 / 4 / 8 envs per
    workgroup up to 512 / 1024 / 2048 envs; (27, 2048, 20) is the HBM-streaming form of the 8-env geometry, (27, 2563, 12)
    the 8-writer-wave instantiation on an ordinary allocation, taken up to 3072 envs), and at 81 /
    243 agents step_kernel's K-loop up to 512 envs, the pipelined kernels from 513 on.  Same bits as K step calls, ragged
    batches and mid-launch resets included."""
    step0 = np.where(np.arange(B) % 4 == 0, 100 - 1 - (np.arange(B) // 4) % K, (np.arange(B) * 7) % (100 - K))
    a, b = _pair(N, B, seed=8, crowd=0.45, step0=step0)
    gen = torch.Generator(device="cuda"); gen.manual_seed(B)
    acts = (torch.rand((K, B, N, 2), generator=gen, device="cuda") * 2 - 1).contiguous()
    saw_done = False
    for launch in range(2):
        obs, rew, done, info = b.rollout(acts)
        saw_done = saw_done or bool(done.any())
        for k in range(K):
            o, r, d, i = a.step(acts[k])
            assert torch.equal(o, obs[k]), "observations differ at step %d of launch %d" % (k, launch)
            assert torch.equal(r, rew[k]) and torch.equal(d, done[k])
            assert torch.equal(i["individual_reward"], info["individual_reward"][k])
        for x, y in zip(a.world.get_state() + (a.scenario.ideal_shape, a.world.step_count),
                        b.world.get_state() + (b.scenario.ideal_shape, b.world.step_count)):
            assert torch.equal(x, y)
    assert saw_done


@pytest.mark.parametrize("B", [300, 700, 1500])
def test_small_batch_closed_loop_rollouts_equal_policy_and_step_calls(B):
    """The closed-loop instantiations of the small-batch geometries (27 agents, 2 / 4 / 8 envs per workgroup)."""
    import formation_gym
    N, K = 27, 6
    a, b = _pair(N, B, seed=10, crowd=0.6, step0=(np.arange(B) * 11) % 100)
    for e in (a, b):
        e.scenario.observe_batch(e.world, {"obs": e._out["obs"], "reward": e._out["reward"]})
    obs, rew, done, info = b.rollout_policy(K, 3)
    o = a._out["obs"]
    for k in range(K):
        act = formation_gym.get_action_BFS(formation_gym.ezpolicy, o, 3)
        assert torch.equal(act, info["actions"][k]), k
        o, r, d, i = a.step(act)
        assert torch.equal(o, obs[k]) and torch.equal(r, rew[k]) and torch.equal(d, done[k])
    for x, y in zip(a.world.get_state(), b.world.get_state()):
        assert torch.equal(x, y)


def test_default_rollout_places_its_buffer_cheaply_and_gives_the_memory_back():
    """env.rollout(action_seq) with no buffers passed (what a caller of the reference's loop does, test.py:14-28): the env
    places its observation buffer on first use - a TIMED choice among compositions of a SMALL arena (<= 6 x the buffer,
    formation_gym/placement.py; the round-3 probe mapped 206 GB) - and re-uses it.  Checked here: the rate against the same
    launch into an ordinary allocation, the memory the probe takes and gives back, the same bits either way, and that the
    arena lives exactly as long as the tensors (placed buffers leaked over the env's lifetime)."""
    import gc
    N, B, K = 27, 4096, 20
    step0 = (np.arange(B) * 7) % 60
    a, b = _pair(N, B, seed=2, crowd=0.5, step0=step0)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    acts = (torch.rand((K, B, N, 2), generator=gen, device="cuda") * 2 - 1).contiguous()
    buffer_bytes = K * B * N * 6 * N * 4
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    obs_b, rew_b, done_b, info_b = b.rollout(acts)                       # places (probe) and launches
    torch.cuda.synchronize()
    rep = b.placement
    assert rep["probed"] and rep["stages"][0]["arena_GB"] * 1e9 <= 6.1 * buffer_bytes and rep["probe_seconds"] < (1.0 if len(rep["stages"]) == 1 else 15.0), rep
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 <= 1.25 * buffer_bytes + (256 << 20), "the probe kept more than the buffer: %.2f GB" % ((free0 - free1) / 1e9)
    f = dict(dtype=torch.float32, device="cuda")
    plain = dict(obs=torch.empty((K, B, N, 6 * N), **f), reward=torch.empty((K, B, N), **f), indiv=torch.empty((K, B, N), **f),
                 done=torch.zeros((K, B, N), dtype=torch.uint8, device="cuda"))
    obs_a, rew_a, done_a, info_a = a.rollout(acts, out=plain)
    assert torch.equal(obs_a, obs_b) and torch.equal(rew_a, rew_b) and torch.equal(done_a, done_b)
    assert torch.equal(info_a["individual_reward"], info_b["individual_reward"])
    assert b.rollout(acts)[0].data_ptr() == obs_b.data_ptr()             # the same buffer again, no second probe

    def rate(env, out):
        for _ in range(10):
            env.rollout(acts, out=out)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(41)]
        ev[0].record()
        for r in range(40):
            env.rollout(acts, out=out)
            ev[r + 1].record()
        torch.cuda.synchronize()
        ts = sorted(ev[r].elapsed_time(ev[r + 1]) for r in range(40))
        return ts[len(ts) // 2]
    t_plain, t_placed = rate(a, plain), rate(b, None)
    t_plain2 = rate(a, plain)
    # never slower than an ordinary allocation (the probe times that composition too); the usual gain is 6-10 %
    # (profiles/r04_place/arena_size.txt), asserted loosely because the ordinary allocation's own rate varies by box
    assert t_placed <= 1.03 * min(t_plain, t_plain2), (t_placed, t_plain, t_plain2)
    print("placed %.4f ms, ordinary %.4f / %.4f ms per %d-step launch; probe: %s" % (t_placed, t_plain, t_plain2, K, rep))
    # lifetime: the arena goes when the last tensor of the buffer goes - not before, not later
    import weakref
    from formation_gym import placement
    live = [r for r in placement._live_arenas if r() is not None and r()._handle is not None]
    assert len(live) >= 1
    view = obs_b[3]
    del obs_b, rew_b, done_b, info_b
    b.close()
    gc.collect()
    assert any(r() is not None and r()._handle is not None for r in live), "the arena went although a view of the buffer is alive"
    view.fill_(1.0); torch.cuda.synchronize()                            # still mapped
    del view
    gc.collect(); torch.cuda.synchronize(); torch.cuda.empty_cache()
    assert all(r() is None or r()._handle is None for r in live)
    a.close()                                                            # its bound launch holds `plain`
    del plain, obs_a, rew_a, done_a, info_a
    gc.collect(); torch.cuda.empty_cache()
    free2 = torch.cuda.mem_get_info()[0]
    assert free2 >= free0 - (64 << 20), "device memory not returned: %.2f GB missing" % ((free0 - free2) / 1e9)


def test_probe_looks_at_more_memory_when_the_first_arena_gains_nothing(monkeypatch):
    """placement.probe_arena escalates - 4 x the arena, twice at most - when its winner is not 8 % faster than the arena's
    first chunks (some boxes' first ~10 GB run every composition of a multi-GB buffer alike and slow: profiles/r04_place/).
    Forced here by asking for an impossible gain: three stages, each arena closed before the next is made, the kept
    buffer usable, every byte back afterwards."""
    import gc
    from formation_gym import placement
    monkeypatch.setattr(placement, "ESCALATE_BELOW_GAIN", 0.0)
    monkeypatch.setattr(placement, "ESCALATE_MIN_BYTES", 0)
    monkeypatch.setattr(placement, "ESCALATE_INSENSITIVE", 0.0)        # (a copy_ does not care where its buffer lies)
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    n = (768 << 20) // 4
    src = torch.ones(n, dtype=torch.float32, device="cuda")
    flat, rep, arena = placement.probe_arena(n, lambda dst: dst.copy_(src), "cuda", trials=4, budget_s=0.1)
    sizes = [s["arena_GB"] for s in rep["stages"]]
    assert len(sizes) == 3 and sizes[1] >= 3.9 * sizes[0] and sizes[2] >= 3.9 * sizes[1], rep
    assert rep["arena_GB"] in sizes and rep["kept_ms"] <= min(s["kept_ms"] for s in rep["stages"]) * 1.0001   # the best stage's winner is kept
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 <= 2 * n * 4 + n * 4 // 4 + (256 << 20), "closed stages still hold memory: %.2f GB" % ((free0 - free1) / 1e9)
    flat.copy_(src); torch.cuda.synchronize()
    assert float(flat.sum()) == float(n)
    del flat
    arena.close()
    del src
    gc.collect(); torch.cuda.empty_cache()
    assert torch.cuda.mem_get_info()[0] >= free0 - (64 << 20)
    # a larger arena that cannot be made: the first stage's winner, which was held meanwhile, is what comes back
    real_stage, calls = placement._probe_stage, []

    def failing_second(geometry, *args, **kw):
        calls.append(geometry[0])
        return None if len(calls) == 2 else real_stage(geometry, *args, **kw)
    monkeypatch.setattr(placement, "_probe_stage", failing_second)
    flat, rep, arena = placement.probe_arena(n, lambda dst: dst.zero_(), "cuda", trials=4, budget_s=0.1)
    assert len(calls) == 2 and calls[1] > 3.9 * calls[0]
    assert len(rep["stages"]) == 2 and rep["stages"][1].get("failed") and rep["arena_GB"] == rep["stages"][0]["arena_GB"]
    flat.fill_(2.0); torch.cuda.synchronize()
    del flat
    arena.close()
    monkeypatch.setattr(placement, "_probe_stage", real_stage)
    # and a caller that names the arena size gets that size, once
    flat, rep, arena = placement.probe_arena(n, lambda dst: dst.zero_(), "cuda", trials=4, budget_s=0.1, max_arena_bytes=2 << 30)
    assert len(rep["stages"]) == 1 and rep["arena_GB"] <= 2.2
    del flat
    arena.close()


# ---- the one bound-launch path of rollout, rollout_policy and rollout_actor ----
_RN, _RB, _RK, _REVERY = 3, 8, 3, 2        # one stored observation, K no multiple of obs_every, an episode end inside the launch


def _small_env(**agent1):
    import formation_gym
    e = formation_gym.make_env("formation_hd_env", False, _RN, num_envs=_RB, device="cuda:0", episode_length=2)
    for k, v in agent1.items():
        setattr(e.world.agents[1], k, v)
    e.seed(5)
    e.reset()
    e.auto_reset = True
    return e


def _small_actor(seed=0):
    torch.manual_seed(seed)
    nn = torch.nn
    return nn.Sequential(nn.Linear(6 * _RN, 32), nn.ReLU(), nn.Linear(32, 32), nn.ReLU(), nn.Linear(32, 2), nn.Tanh()).to("cuda:0")


def _flat(res):
    """Everything a K-step call returns, by name, cloned."""
    obs, rew, done, info = res
    return dict({"obs": obs.clone(), "reward": rew.clone(), "done": done.clone()}, **{k: v.clone() for k, v in info.items()})


@pytest.mark.parametrize("kind", ["rollout", "rollout_policy", "rollout_actor"])
def test_the_three_rollouts_share_one_cache_rule(kind):
    """A caller's `out` is bound once and re-used, every other `out` dict is one more binding, out=False and a dict that
    lacks an optional tensor are never cached, the cache is cleared when it holds 8, and a cached launch returns the bits of an
    uncached one from the same state."""
    from formation_gym import GaussianActor
    e = _small_env()
    actor = _small_actor()
    acts = torch.rand((_RK, _RB, _RN, 2), device="cuda:0") * 2 - 1

    def call(out, actor=actor):
        if kind == "rollout":
            return e.rollout(acts, out=out, obs_every=_REVERY)
        if kind == "rollout_policy":
            return e.rollout_policy(_RK, 3, out=out, obs_every=_REVERY)
        return e.rollout_actor(_RK, actor, out=out, obs_every=_REVERY)

    def buffers():
        return e.alloc_rollout_buffers(_RK, obs_every=_REVERY, policy=kind != "rollout")

    outs = [buffers() for _ in range(9)]
    e._roll_launchers.clear()
    snap = e._snapshot()
    call(outs[0])
    assert len(e._roll_launchers) == 1
    e._restore(snap)
    cached = _flat(call(outs[0]))
    assert len(e._roll_launchers) == 1
    assert bool(cached["done"].any()) and not bool(cached["done"].all()), "no episode end inside the launch"
    e._restore(snap)
    fresh = _flat(call(False))
    assert len(e._roll_launchers) == 1
    assert sorted(fresh) == sorted(cached) and ("actions" in fresh) == (kind != "rollout")
    assert fresh["obs"].shape[0] == _RK // _REVERY
    for k in fresh:
        assert torch.equal(fresh[k], cached[k]), k
    call(outs[1])
    assert len(e._roll_launchers) == 2
    if kind == "rollout_actor":
        assert "log_prob" not in outs[0]
        info = call(outs[0], GaussianActor(actor).to("cuda:0"))[3]
        assert info["log_prob"].shape == (_RK, _RB, _RN) and len(e._roll_launchers) == 2
    for out in outs[2:8]:
        call(out)
    assert len(e._roll_launchers) == 8
    call(outs[8])
    assert len(e._roll_launchers) == 1
    torch.cuda.synchronize()


def test_a_mass_edit_and_back_reads_the_live_agent_table():
    """Agent 1's mass A -> B -> A with bound steps and a bound rollout in every phase: the bindings of the first phase are
    selected again in the last (the launcher caches key on the world's signature) and must read a per-agent table that is still
    alive, not the block the second phase's table freed.  Against a fresh env of mass A in the same state."""
    A, B_ = 2.0, 3.0
    e = _small_env(initial_mass=A)
    act = torch.rand((_RB, _RN, 2), device="cuda:0") * 2 - 1
    acts = torch.rand((_RK, _RB, _RN, 2), device="cuda:0") * 2 - 1
    out = e.alloc_rollout_buffers(_RK, obs_every=_REVERY)

    def phase(env, out):
        res = [_flat(env.step(act)), _flat(env.step(act)), _flat(env.rollout(acts, out=out, obs_every=_REVERY))]
        return [{k: r[k] for k in ("obs", "reward", "individual_reward", "done")} for r in res]

    phase(e, out)
    assert len(e._launchers) == 1 and len(e._roll_launchers) == 1
    e.world.agents[1].initial_mass = B_
    phase(e, out)
    junk = [torch.full((_RN, 8), 50.0, device="cuda:0") for _ in range(4)]      # what the allocator may put where table A was
    e.world.agents[1].initial_mass = A
    ref = _small_env(initial_mass=A)
    ref._restore(e._snapshot())
    got = phase(e, out)
    assert len(e._launchers) == 2 and len(e._roll_launchers) == 2, "the last phase re-uses the first phase's bindings"
    want = phase(ref, ref.alloc_rollout_buffers(_RK, obs_every=_REVERY))
    for g, w in zip(got, want):
        for k in w:
            assert torch.equal(g[k], w[k]), k
    del junk
