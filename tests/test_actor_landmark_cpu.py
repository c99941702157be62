"""CPU checks of the learned-actor rollout in the landmark scenarios (`fg_rollout_scenario_actor`): which path an actor takes,
the dry-run description of the fused launch, argument checks that touch no device, and the new kernels' resources."""
import ctypes
import types

import pytest
import torch

from formation_gym import _native, actor_rollout, load_scenario
from formation_gym.actor_rollout import (FUSED_HIDDEN, FUSED_N, LANDMARK_FUSED_HIDDEN, LANDMARK_FUSED_SHAPES, GaussianActor,
                                         PerAgentActor, actor_path, actor_spec, landmark_facts, sample_spec)
from tests.actor_testlib import LIB, describe, fake_actor as _fake_actor, params

# (scenario file, agents, landmarks, obstacles, num_obs) of the seven shapes, and the observation width the kernel composes
SHAPES = [("basic_formation_env", 3, 3, 0, 0, 18), ("formation_hd_partial_env", 5, 5, 0, 3, 26),
          ("formation_hd_partial_env", 3, 5, 0, 3, 22), ("formation_hd_partial_range_env", 4, 4, 0, 0, 22),
          ("formation_hd_partial_range_env", 3, 4, 0, 0, 18), ("formation_hd_obs_env", 4, 4, 3, 0, 28),
          ("formation_hd_obs_env", 3, 4, 3, 0, 24)]


def _mlp(D, H, tanh=True, bias=True, dtype=torch.float32):
    mods = [torch.nn.Linear(D, H, bias=bias), torch.nn.ReLU(), torch.nn.Linear(H, H), torch.nn.ReLU(),
            torch.nn.Linear(H, 2, bias=bias)]
    if tanh:
        mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods).to(dtype)


def _scenario(name, N, L, M, num_obs, variant=0):
    """The scenario object and a stand-in world (agents and landmarks only): what `actor_fused_rule` looks at, no device."""
    sc = load_scenario(name)
    world = types.SimpleNamespace(agents=[None] * N, landmarks=[None] * (L + M))
    sc.num_agents, sc.num_landmarks, sc.num_obstacles, sc.num_obs, sc.obs_range = N, L, M, num_obs, 0.0
    if variant:
        sc.kernel_variant = variant
    return sc, world


def _path(sc, world, actor, **env_facts):
    """MultiAgentEnv.actor_path's decision from the scenario's rule and the env's facts."""
    facts = sc.actor_fused_rule(world)
    if facts is None:
        return actor_path(actor, len(world.agents), fused_scenario=False, **env_facts)
    return actor_path(actor, len(world.agents), fused_scenario=True, **env_facts, **facts)


@pytest.mark.parametrize("name,N,L,M,num_obs,D", SHAPES)
def test_landmark_shapes_fuse(name, N, L, M, num_obs, D):
    sc, world = _scenario(name, N, L, M, num_obs)
    assert sc.obs_dim(world) == D
    for H in LANDMARK_FUSED_HIDDEN:
        for tanh in (True, False):
            for bias in (True, False):
                actor = _mlp(D, H, tanh, bias)
                assert _path(sc, world, actor) == "fused", (H, tanh, bias)
                assert _path(sc, world, GaussianActor(actor)) == "fused"
                facts = {k: v for k, v in sc.actor_fused_rule(world).items() if k != "per_agent"}
                hidden, out_tanh, ws = actor_spec(actor, N, **facts)
                assert (hidden, out_tanh) == (H, tanh) and len(ws) == 6 and (ws[1] is None) == (not bias)
                assert sample_spec(GaussianActor(actor), N, **facts)[0][0] == H
    good = _mlp(D, 64)
    assert _path(sc, world, _mlp(D, 128)) == "host"                                  # H = 128 stays host-paced here
    assert _path(sc, world, GaussianActor(_mlp(D, 128))) == "host"
    assert _path(sc, world, _mlp(D + 2, 64)) == "host"                               # a wrong input width
    if 6 * N != D:                                                                    # (basic, range at 3 agents: 6N = 18 = D)
        assert _path(sc, world, _mlp(6 * N, 64)) == "host"                           # formation_hd_env's input width
    assert _path(sc, world, PerAgentActor([_mlp(D, 64) for _ in range(N)])) == "host"
    assert _path(sc, world, GaussianActor(PerAgentActor([_mlp(D, 64) for _ in range(N)]))) == "host"
    assert _path(sc, world, _mlp(D, 64, dtype=torch.float64)) == "host"
    strided = _mlp(D, 64)
    strided[2].weight = torch.nn.Parameter(torch.zeros(64, 128)[:, ::2])            # non-contiguous
    assert _path(sc, world, strided) == "host"
    assert _path(sc, world, lambda o: o[..., :2]) == "host"
    # the env's facts, as MultiAgentEnv.actor_path derives them: walls / u_noise / per-agent mass (agent_props) are World
    # options; a discrete action mode; non-silent agents; a post_step_callback
    assert _path(sc, world, good, world_options=True) == "host"
    assert _path(sc, world, good, continuous=False) == "host"
    assert _path(sc, world, good, silent=False) == "host"
    assert _path(sc, world, good, callback=True) == "host"
    assert _path(sc, world, good, device="cuda:0") == "host"                         # parameters not on the env's device
    # the run-time-count kernel
    sc1, world1 = _scenario(name, N, L, M, num_obs, variant=1)
    assert sc1.actor_fused_rule(world1) is None and _path(sc1, world1, good) == "host"


def test_other_agent_counts_run_host_paced():
    for name, N, L, M, num_obs in (("basic_formation_env", 4, 4, 0, 0), ("basic_formation_env", 3, 4, 0, 0),
                                   ("formation_hd_partial_env", 4, 4, 0, 3), ("formation_hd_partial_env", 5, 5, 0, 2),
                                   ("formation_hd_partial_range_env", 5, 5, 0, 0), ("formation_hd_obs_env", 4, 4, 2, 0)):
        sc, world = _scenario(name, N, L, M, num_obs)
        assert sc.actor_fused_rule(world) is None, (name, N, L, M)
        assert _path(sc, world, _mlp(sc.obs_dim(world), 64)) == "host"
    assert len(LANDMARK_FUSED_SHAPES) == 7
    assert landmark_facts(1, 3, 3, 0, 0, 18) == dict(in_features=18, fused_n=(3,), fused_hidden=(32, 64), per_agent=False)


def test_environment_uses_the_scenario_rule():
    """MultiAgentEnv.actor_path / rollout_actor on a stand-in env (no device): the scenario's facts reach actor_path."""
    from formation_gym.environment import MultiAgentEnv
    sc, world = _scenario("formation_hd_obs_env", 4, 4, 3, 0)
    world.device = None
    world.any_non_silent = lambda: False
    sc.params = lambda w: types.SimpleNamespace(num_walls=0, u_noise=0.0, max_speed=0.0, accel=0.0, agent_props=None,
                                                comm_state=None)
    env = types.SimpleNamespace(scenario=sc, world=world, num_agents=4, post_step_callback=None, _action_mode=lambda: 0)
    env._actor_facts = lambda: MultiAgentEnv._actor_facts(env)
    env._resolve_actor = lambda actor: MultiAgentEnv._resolve_actor(env, actor)
    assert MultiAgentEnv.actor_path(env, _mlp(28, 64)) == "fused"
    assert MultiAgentEnv.actor_path(env, _mlp(24, 64)) == "host"
    assert MultiAgentEnv.actor_path(env, PerAgentActor([_mlp(28, 64) for _ in range(4)])) == "host"
    sc.params = lambda w: types.SimpleNamespace(num_walls=2, u_noise=0.0, max_speed=0.0, accel=0.0, agent_props=None,
                                                comm_state=None)
    assert MultiAgentEnv.actor_path(env, _mlp(28, 64)) == "host"                   # walls
    sc.params = lambda w: types.SimpleNamespace(num_walls=0, u_noise=0.0, max_speed=0.0, accel=0.0, agent_props=4096,
                                                comm_state=None)
    assert MultiAgentEnv.actor_path(env, _mlp(28, 64)) == "host"                   # per-agent mass: World.agent_props
    env.post_step_callback = lambda *a: None
    assert MultiAgentEnv.actor_path(env, _mlp(28, 64)) == "host"


def test_formation_hd_decisions_unchanged():
    """The old call signatures give the old answers."""
    for N in FUSED_N:
        for H in FUSED_HIDDEN:
            actor = _mlp(6 * N, H)
            assert actor_path(actor, N) == "fused"
            assert actor_spec(actor, N)[0] == H and actor_spec(actor, N, None)[0] == H
            assert actor_path(GaussianActor(actor), N) == "fused" and sample_spec(GaussianActor(actor), N)[0][0] == H
    assert (FUSED_N, FUSED_HIDDEN) == ((3, 4, 8, 9, 16, 25, 27, 32), (32, 64, 128))
    assert actor_path(PerAgentActor([_mlp(54, 64) for _ in range(9)]), 9) == "fused"
    assert actor_path(GaussianActor(PerAgentActor([_mlp(54, 64) for _ in range(9)])), 9) == "fused"
    assert actor_path(_mlp(54, 48), 9) == "host"
    assert actor_path(_mlp(18, 64), 9) == "host"                # a landmark width is not formation_hd_env's
    assert actor_path(_mlp(6 * 5, 64), 5) == "host" and actor_spec(_mlp(6 * 5, 64), 5) is None
    assert actor_path(_mlp(54, 64), 9, fused_scenario=False) == "host"
    assert actor_path(_mlp(54, 64), 9, world_options=True) == "host"


def _params():
    return params(dist_min=0.2, collide_thresh=0.2, world_length=50)


KIND = {"basic_formation_env": _native.FG_SCN_BASIC, "formation_hd_partial_env": _native.FG_SCN_PARTIAL,
        "formation_hd_partial_range_env": _native.FG_SCN_RANGE, "formation_hd_obs_env": _native.FG_SCN_OBSTACLE}


def _desc(name, L, M, num_obs, variant=0):
    return _native.FgScenario(kind=KIND[name], num_landmarks=L, num_obstacles=M, num_obs=num_obs, obs_range=1.0,
                              obstacle_size=0.15, obstacle_vx=0.0, obstacle_vy=-1.0, obstacle_floor=-2.2, penalty=1.0,
                              variant=variant)


def _describe(lib, name, N, L, M, num_obs, H, sample, B=4096, K=20, params=None, variant=0):
    lead = (_desc(name, L, M, num_obs, variant), _fake_actor(H), ctypes.c_void_p(4096) if sample else None)
    return describe(lib, "fg_describe_scenario_actor_launch", lead, N, B, K, params or _params())


def test_describe_names_one_instantiation_per_shape():
    lib = _native.load()
    names = set()
    for name, N, L, M, num_obs, D in SHAPES:
        for H in LANDMARK_FUSED_HIDDEN:
            for sample in (False, True):
                rc, text = _describe(lib, name, N, L, M, num_obs, H, sample)
                assert rc == 0, text
                kernel = "scn_lane_actor_gauss<" if sample else "scn_lane_actor<"
                nbr = num_obs if name == "formation_hd_partial_env" else N - 1
                assert text.startswith("%s%d,%d,%d,%d,%d,%d>" % (kernel, KIND[name], N, L, M, nbr, H)), text
                # geometry: 256 threads = 64 envs per workgroup, the grid rounded up to the 8 XCDs
                assert "grid 64 threads 256 envs/wg 64 lds " in text, text
                assert int(text.split("lds ")[1].split(";")[0]) <= 160 * 1024
                for other in ("actor_rollout_kernel", "actor_sample_kernel", "pa_actor_kernel", "pa_sample_kernel"):
                    assert other not in text
                names.add(text.split(" ")[0])
    assert len(names) == 28
    rc, text = _describe(lib, "basic_formation_env", 3, 3, 0, 0, 64, False, B=133)
    assert rc == 0 and "grid 8 " in text                                        # 3 workgroups, a multiple of 8 launched


def test_bad_arguments_rejected_without_a_device():
    lib = _native.load()
    f = ctypes.c_void_p(4096)

    def call(name="basic_formation_env", N=3, L=3, M=0, num_obs=0, K=20, B=128, actor=None, log_std=None, logp=None,
             params=None, variant=0, ptrs=None, act_out=f, obs=f):
        state = ptrs if ptrs is not None else [f] * 8           # pos_x .. vel_y, landmarks, obst_pos, obst_vel, step
        return lib.fg_rollout_scenario_actor(params or _params(), _desc(name, L, M, num_obs, variant),
                                             actor if actor is not None else _fake_actor(64), log_std, B, N, K, *state,
                                             obs, f, f, f, act_out, logp, 1, None)
    assert call(actor=_fake_actor(48)) == -1                                  # FG_ERR_BAD_ARG: hidden width
    assert b"hidden" in lib.fg_last_error()
    assert call(actor=_fake_actor(128)) == -1                                 # H = 128 has no landmark instantiation
    assert b"hidden" in lib.fg_last_error()
    assert call(N=4, L=4) == -2                                               # FG_ERR_UNSUPPORTED_N: basic with 4 agents
    assert call(name="formation_hd_partial_env", N=5, L=5, num_obs=2) == -2
    assert call(name="formation_hd_obs_env", N=4, L=4, M=2) == -2
    no_w1 = _fake_actor(64)
    no_w1.w1 = None
    assert call(actor=no_w1) == -1
    assert call(K=0) == -1 and call(B=-1) == -1
    assert call(ptrs=[None] + [f] * 7) == -1                                  # pos_x
    assert call(ptrs=[f] * 4 + [None] + [f] * 3) == -1                        # landmarks
    assert call(act_out=None) == -1
    assert call(name="formation_hd_obs_env", N=4, L=4, M=3, ptrs=[f] * 5 + [None, None, f]) == -1    # obstacles required
    assert call(logp=f) == -1                                                 # log-probs without log_std
    assert call(variant=1) == -1
    props = _params()
    props.agent_props = 4096
    assert call(params=props) == -1
    comm = _params()
    comm.comm_state = 4096
    assert call(params=comm) == -1
    assert call(act_out=ctypes.c_void_p(4100)) == -3                          # FG_ERR_ALIGNMENT
    assert call(obs=ctypes.c_void_p(4100)) == -3
    assert call(log_std=ctypes.c_void_p(4098)) == -3
    odd = _fake_actor(64)
    odd.w2 = 4098
    assert call(actor=odd) == -3
    assert call(B=0) == 0                                                     # an empty batch: no launch
    assert call(B=0, N=4, L=4) == -2
    rc, _ = _describe(lib, "basic_formation_env", 4, 4, 0, 0, 64, False)
    assert rc == -2
    rc, _ = _describe(lib, "basic_formation_env", 3, 3, 0, 0, 128, True)
    assert rc == -1
    rc, _ = _describe(lib, "basic_formation_env", 3, 3, 0, 0, 64, False, variant=1)
    assert rc == -1
    rc, _ = _describe(lib, "basic_formation_env", 3, 3, 0, 0, 64, False, B=0)
    assert rc == -1


def test_landmark_actor_kernels_resources():
    """No scratch, no spilled VGPRs, fp32 MFMA, no atomics.  The VGPR budget the geometry depends on: a 256-thread workgroup
    puts ONE wave on each SIMD, so a lane may address all 512 registers (256 architectural + 256 accumulation); above 512 the
    kernel could not launch, and up to 512 the LDS footprint (36-74 KiB), not the registers, limits workgroups per CU to two -
    a second workgroup per CU needs <= 256 registers, which the widest shapes (obstacle, H = 64) exceed and run one workgroup
    per CU for; that is recorded in profiles/actor_landmark.md, not asserted."""
    from tests.isa_scan import kernel_disassembly, kernel_resources
    ks = [k for k in kernel_resources(LIB) if "scn_lane_actor" in k["demangled"]]
    assert len(ks) == 28
    assert len([k for k in ks if "scn_lane_actor<" in k["demangled"]]) == 14
    assert len([k for k in ks if "scn_lane_actor_gauss<" in k["demangled"]]) == 14
    for k in ks:
        assert k["private_segment"] == 0 and k["vgpr_spill"] == 0, k
        assert k["vgpr"] <= 512, k
    # instruction scan of the 28 kernels' code
    wanted = {k["name"] for k in ks}
    seen = {name: {"mfma": sum("v_mfma_f32_16x16x4" in ins for ins in code), "atomic": sum("atomic" in ins for ins in code)}
            for name, code in kernel_disassembly(LIB).items() if name in wanted}
    assert set(seen) == wanted
    for name, c in seen.items():
        assert c["mfma"] > 0 and c["atomic"] == 0, (name, c)


def test_native_binding_lists_the_new_symbols():
    lib = _native.load()
    for name in ("fg_rollout_scenario_actor", "fg_describe_scenario_actor_launch"):
        assert name in _native.SIGNATURES and getattr(lib, name) is not None
    assert lib.fg_abi_version() == 8
    assert hasattr(actor_rollout, "LANDMARK_FUSED_SHAPES")
