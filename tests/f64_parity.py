"""Test-side binding of libformation_hip_f64.so, the fp64 "parity mode" build of the fused step kernel
(gym-formation_amd/csrc/formation_hip_f64.hip: the SAME kernel source as the product library with real = double).
Test infrastructure only - the product package never loads it."""
import ctypes
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "gym-formation_amd", "lib", "libformation_hip_f64.so")


class Fg64Params(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("dt", "damping", "contact_force", "contact_margin", "sensitivity", "mass",
                                               "dist_min", "collide_thresh")] + \
               [("world_length", ctypes.c_int32), ("reserved", ctypes.c_int32)]


MAX_WALLS, AGENT_PROPS = 4, 8                                            # FG_MAX_WALLS, FG_AGENT_PROPS (include/formation_hip.h)
AGENT_IMMOVABLE, AGENT_NO_COLLIDE, AGENT_GHOST, AGENT_SCRIPTED = 1, 2, 4, 8


class Fg64Wall(ctypes.Structure):
    _fields_ = [("vertical", ctypes.c_int32), ("soft", ctypes.c_int32)] + \
               [(k, ctypes.c_double) for k in ("axis_pos", "end0", "end1", "width")]


class Fg64Options(ctypes.Structure):
    _fields_ = [("accel", ctypes.c_double), ("max_speed", ctypes.c_double), ("num_walls", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("walls", Fg64Wall * MAX_WALLS), ("agent_props", ctypes.c_void_p),
                ("comm_state", ctypes.c_void_p)]


class Fg64Scenario(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("kind", "num_landmarks", "num_obstacles", "num_obs")] + \
               [(k, ctypes.c_double) for k in ("obs_range", "obstacle_size", "obstacle_vx", "obstacle_vy", "obstacle_floor", "penalty")]


SCN_KINDS = {"basic": 1, "partial": 2, "range": 3, "obstacle": 4}            # FgScenarioKind (include/formation_hip.h)

_lib = None


def load():
    global _lib
    if _lib is None:
        lib = ctypes.CDLL(LIB_PATH)
        lib.fg64_step_hd.restype = ctypes.c_int
        lib.fg64_step_hd.argtypes = [ctypes.POINTER(Fg64Params), ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 16
        lib.fg64_step_hd_opts.restype = ctypes.c_int
        lib.fg64_step_hd_opts.argtypes = [ctypes.POINTER(Fg64Params), ctypes.POINTER(Fg64Options)] + [ctypes.c_int] * 3 + \
                                         [ctypes.c_void_p] * 16
        lib.fg64_rollout_hd.restype = ctypes.c_int
        lib.fg64_rollout_hd.argtypes = [ctypes.POINTER(Fg64Params), ctypes.c_int, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 13
        lib.fg64_rollout_scenario.restype = ctypes.c_int
        lib.fg64_rollout_scenario.argtypes = [ctypes.POINTER(Fg64Params), ctypes.POINTER(Fg64Scenario), ctypes.POINTER(Fg64Options)] + \
                                             [ctypes.c_int] * 6 + [ctypes.c_void_p] * 15
        lib.fg64_rollout_hd_returns.restype = ctypes.c_int
        lib.fg64_rollout_hd_returns.argtypes = [ctypes.POINTER(Fg64Params)] + [ctypes.c_int] * 4 + [ctypes.c_double] + \
                                               [ctypes.c_void_p] * 12
        _lib = lib
    return _lib


def default_params(**kw):
    """The constants in force at the BASELINE configs, in double."""
    d = dict(dt=0.1, damping=0.25, contact_force=1e2, contact_margin=1e-3, sensitivity=5.0, mass=1.0,
             dist_min=0.06, collide_thresh=0.03, world_length=100)
    d.update(kw)
    return Fg64Params(**d)


def params_of(P):
    """Fg64Params of an oracle parameter object (oracle.formation_oracle.HdParams): the same doubles"""
    return default_params(dt=P.dt, damping=P.damping, contact_force=P.contact_force, contact_margin=P.contact_margin,
                          sensitivity=P.sensitivity, mass=P.mass, dist_min=P.dist_min, collide_thresh=P.collide_thresh,
                          world_length=P.world_length)


def kernel_options(N, P, mass=None, size=None, accel=None, max_speed=None, walls=None, movable=None, collide=None, ghost=None,
                   scripted=None):
    """The oracle's World options (keyword arguments of O.physics_step) as the kernel takes them:
    dict(accel, max_speed, walls, agent_props[, sensitivity]).  accel / max_speed given as one number stay the World-wide scalars; anything per
    agent makes the [N][8] table (NaN = None = 0), whose columns are FgParams.agent_props'."""
    per_agent = any(x is not None for x in (mass, size, movable, collide, ghost, scripted)) or \
        any(x is not None and np.ndim(x) > 0 for x in (accel, max_speed))
    o = dict(accel=0.0, max_speed=0.0, agent_props=None, walls=[])
    for w in walls or []:
        o["walls"].append(dict(vertical=int(w[0] == "V"), axis_pos=float(w[1]), end0=float(w[2][0]), end1=float(w[2][1]),
                               width=float(w[3]), soft=int(len(w) > 4 and not w[4])))
    if not per_agent:
        o["accel"] = 0.0 if accel is None else float(accel)
        # FgParams' contract for a World-wide accel: `sensitivity` carries it too (environment.py:218-220; the product's
        # World.native_params and INTEGRATION.md's example fill it so) - the kernel multiplies mass * accel * (sensitivity * u)
        o["sensitivity"] = None if accel is None else float(accel)
        o["max_speed"] = 0.0 if max_speed is None else float(max_speed)
        return o
    col = lambda x, default: np.broadcast_to(np.asarray(default if x is None else x, dtype=np.float64), (N,))
    t = np.zeros((N, AGENT_PROPS))
    t[:, 0] = col(mass, P.mass)
    t[:, 1] = col(size, P.agent_size)
    t[:, 2] = np.nan_to_num(col(accel, np.nan), nan=0.0)
    t[:, 3] = np.nan_to_num(col(max_speed, np.nan), nan=0.0)
    flag = lambda x, default: np.broadcast_to(np.asarray(default if x is None else x, dtype=bool), (N,))
    t[:, 6] = (AGENT_IMMOVABLE * ~flag(movable, True) + AGENT_NO_COLLIDE * ~flag(collide, True) + AGENT_GHOST * flag(ghost, False) +
               AGENT_SCRIPTED * flag(scripted, False))
    o["agent_props"] = t
    return o


class Env64(object):
    """B envs of N agents held in fp64 device tensors; `step(act)` = one fg64_step_hd launch.
    options: dict(accel, max_speed, walls, agent_props) as kernel_options() makes it -> every launch goes through
    fg64_step_hd_opts (step_kernel's OPTS instantiation): `step(act, comm)` with that step's communication states [B,N,2], or
    `rollout(acts)`, K steps in ONE launch through the kernel's own K-loop."""

    def __init__(self, pos, vel, ideal_shape, ideal_vel, step=None, params=None, indices=True, options=None):
        f = dict(dtype=torch.float64, device="cuda")
        pos = np.asarray(pos, dtype=np.float64)
        self.B, self.N = pos.shape[:2]
        B, N = self.B, self.N
        self.px = torch.as_tensor(np.ascontiguousarray(pos[..., 0]), **f)
        self.py = torch.as_tensor(np.ascontiguousarray(pos[..., 1]), **f)
        vel = np.asarray(vel, dtype=np.float64)
        self.vx = torch.as_tensor(np.ascontiguousarray(vel[..., 0]), **f)
        self.vy = torch.as_tensor(np.ascontiguousarray(vel[..., 1]), **f)
        self.shape = torch.as_tensor(np.array(np.broadcast_to(ideal_shape, (B, N, 2))), **f)
        self.ivel = torch.as_tensor(np.array(np.broadcast_to(ideal_vel, (B, 2))), **f)
        self.step_count = torch.as_tensor(np.zeros(B, dtype=np.int32) if step is None else np.asarray(step, dtype=np.int32)).cuda()
        self.obs = torch.empty((B, N, 6 * N), **f)
        self.reward = torch.empty((B, N), **f)
        self.indiv = torch.empty((B, N), **f)
        self.done = torch.zeros((B, N), dtype=torch.uint8, device="cuda")
        self.near_lm = torch.zeros((B, N), dtype=torch.int32, device="cuda") if indices else None
        self.near_ag = torch.zeros((B, N), dtype=torch.int32, device="cuda") if indices else None
        self.hd_idx = torch.zeros((B, 4), dtype=torch.int32, device="cuda") if indices else None
        self.params = params or default_params()
        self.options = None
        if options is not None:
            o = Fg64Options(accel=options.get("accel", 0.0), max_speed=options.get("max_speed", 0.0),
                            num_walls=len(options.get("walls") or []))
            assert o.num_walls <= MAX_WALLS
            for k, w in enumerate(options.get("walls") or []):
                o.walls[k] = Fg64Wall(**w)
            self.props = None
            if options.get("agent_props") is not None:
                t = np.ascontiguousarray(options["agent_props"], dtype=np.float64)
                assert t.shape == (N, AGENT_PROPS)
                self.props = torch.as_tensor(t, **f)
                o.agent_props = self.props.data_ptr()
            self.options = o
            if options.get("sensitivity") is not None:
                self.params = Fg64Params.from_buffer_copy(self.params)
                self.params.sensitivity = options["sensitivity"]

    def _launch_opts(self, act, K, obs, reward, indiv, done, comm):
        """fg64_step_hd_opts over act [K,B,N,2] into obs [K,B,N,6N], reward / indiv / done [K,B,N]"""
        f = dict(dtype=torch.float64, device="cuda")
        p = lambda t: None if t is None else t.data_ptr()
        self.comm = None if comm is None else torch.as_tensor(np.ascontiguousarray(comm, dtype=np.float64), **f)
        assert self.comm is None or tuple(self.comm.shape) == (self.B, self.N, 2)
        self.options.comm_state = p(self.comm)
        rc = load().fg64_step_hd_opts(self.params, self.options, self.B, self.N, K, p(self.px), p(self.py), p(self.vx), p(self.vy),
                                      p(act), p(self.shape), p(self.ivel), p(self.step_count), p(obs), p(reward), p(indiv), p(done),
                                      p(self.near_lm), p(self.near_ag), p(self.hd_idx), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, "fg64_step_hd_opts returned %d" % rc
        torch.cuda.synchronize()

    def rollout(self, acts):
        """K = len(acts) steps in ONE fg64_step_hd_opts launch.  Returns dict(obs [K,B,N,6N], reward, indiv, done [K,B,N])."""
        f = dict(dtype=torch.float64, device="cuda")
        acts = torch.as_tensor(np.ascontiguousarray(np.asarray(acts, dtype=np.float64)), **f)
        K, B, N = acts.shape[0], self.B, self.N
        assert tuple(acts.shape) == (K, B, N, 2)
        obs = torch.full((K, B, N, 6 * N), float("nan"), **f)
        rew = torch.full((K, B, N), float("nan"), **f)
        indiv = torch.full((K, B, N), float("nan"), **f)
        done = torch.full((K, B, N), 7, dtype=torch.uint8, device="cuda")
        self._launch_opts(acts, K, obs, rew, indiv, done, None)
        return dict(obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), indiv=indiv.cpu().numpy(), done=done.cpu().numpy())

    def step(self, act, comm=None):
        act = torch.as_tensor(np.ascontiguousarray(np.asarray(act, dtype=np.float64)), dtype=torch.float64, device="cuda")
        p = lambda t: None if t is None else t.data_ptr()
        if self.options is not None:
            assert tuple(act.shape) == (self.B, self.N, 2)
            self._launch_opts(act, 1, self.obs, self.reward, self.indiv, self.done, comm)
            return self
        assert comm is None, "communication states need the options entry"
        rc = load().fg64_step_hd(self.params, self.B, self.N, p(self.px), p(self.py), p(self.vx), p(self.vy), p(act),
                                 p(self.shape), p(self.ivel), p(self.step_count), p(self.obs), p(self.reward),
                                 p(self.indiv), p(self.done), p(self.near_lm), p(self.near_ag), p(self.hd_idx),
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0, "fg64_step_hd returned %d" % rc
        torch.cuda.synchronize()
        return self

    def pos(self):
        return torch.stack((self.px, self.py), -1).cpu().numpy()

    def vel(self):
        return torch.stack((self.vx, self.vy), -1).cpu().numpy()


def scenario_of(kind, P):
    """Fg64Scenario of an oracle parameter object (O.BasicParams / O.ScnParams): the same doubles"""
    if kind == "basic":
        return Fg64Scenario(kind=SCN_KINDS[kind], num_landmarks=P.num_landmarks, num_obstacles=0, num_obs=0, obs_range=0.0,
                            obstacle_size=0.0, obstacle_vx=0.0, obstacle_vy=0.0, obstacle_floor=0.0, penalty=1.0)
    return Fg64Scenario(kind=SCN_KINDS[kind], num_landmarks=P.num_landmarks, num_obstacles=P.num_obstacles, num_obs=P.num_obs,
                        obs_range=P.obs_range, obstacle_size=P.obstacle_size, obstacle_vx=P.obstacle_vel[0],
                        obstacle_vy=P.obstacle_vel[1], obstacle_floor=P.obstacle_floor, penalty=P.penalty)


SENTINEL = -7.5e33          # fill of every float output before a launch: a value no scenario produces


class Scn64(object):
    """B envs of a landmark scenario (kind: basic / partial / range / obstacle) held in fp64 device tensors; `rollout(acts)` = ONE
    fg64_rollout_scenario launch of K = len(acts) steps through scn_kernel's own K-loop, `step(act)` = a launch with K = 1.
    state: dict(pos, vel [B,N,2], landmarks [B,L,2], obst_pos, obst_vel [B,M,2] (obstacle), step [B]); P: the oracle's parameter
    object; options: as kernel_options() makes them; stage: which observation writer (0 straight to memory, 1 through LDS)."""

    def __init__(self, kind, state, P, options=None, stage=0):
        f = dict(dtype=torch.float64, device="cuda")
        dev = lambda x: torch.as_tensor(np.ascontiguousarray(np.asarray(x, dtype=np.float64)), **f)
        pos, vel = np.asarray(state["pos"], dtype=np.float64), np.asarray(state["vel"], dtype=np.float64)
        self.kind, self.stage = kind, int(stage)
        self.B, self.N = pos.shape[:2]
        self.px, self.py, self.vx, self.vy = dev(pos[..., 0]), dev(pos[..., 1]), dev(vel[..., 0]), dev(vel[..., 1])
        self.lm = dev(state["landmarks"])
        self.L = self.lm.shape[1]
        self.M = P.num_obstacles if kind == "obstacle" else 0
        self.opos = dev(state["obst_pos"]) if self.M else None
        self.ovel = dev(state["obst_vel"]) if self.M else None
        assert tuple(self.lm.shape) == (self.B, self.L, 2) and (not self.M or tuple(self.opos.shape) == (self.B, self.M, 2))
        self.step_count = torch.as_tensor(np.ascontiguousarray(np.asarray(state["step"], dtype=np.int32))).cuda()
        self.params = params_of(P)
        self.scenario = scenario_of(kind, P)
        nbr = P.num_obs if kind == "partial" else self.N - 1
        self.D = 2 + (2 if kind == "basic" else 0) + 2 * self.L + 2 * self.M + 2 * nbr + 2 * (self.N - 1)
        options = options or {}
        o = Fg64Options(accel=options.get("accel", 0.0), max_speed=options.get("max_speed", 0.0), num_walls=len(options.get("walls") or []))
        assert o.num_walls <= MAX_WALLS
        for k, w in enumerate(options.get("walls") or []):
            o.walls[k] = Fg64Wall(**w)
        self.props = None
        if options.get("agent_props") is not None:
            t = np.ascontiguousarray(options["agent_props"], dtype=np.float64)
            assert t.shape == (self.N, AGENT_PROPS)
            self.props = torch.as_tensor(t, **f)
            o.agent_props = self.props.data_ptr()
        self.options = o
        if options.get("sensitivity") is not None:
            self.params.sensitivity = options["sensitivity"]

    def launch(self, acts, obs_every=1, do_physics=1):
        """The raw return code and the outputs of one launch over acts [K,B,N,2]: (rc, dict(obs [K / obs_every,B,N,D], reward, indiv,
        done [K,B,N], near_ag [K,B,L] for basic)).  Every output is filled with a sentinel (SENTINEL / 7 / -1) beforehand."""
        f = dict(dtype=torch.float64, device="cuda")
        acts = torch.as_tensor(np.ascontiguousarray(np.asarray(acts, dtype=np.float64)), **f)
        K, B, N = acts.shape[0], self.B, self.N
        assert tuple(acts.shape) == (K, B, N, 2)
        out = dict(obs=torch.full((K // max(obs_every, 1), B, N, self.D), SENTINEL, **f), reward=torch.full((K, B, N), SENTINEL, **f),
                   indiv=torch.full((K, B, N), SENTINEL, **f), done=torch.full((K, B, N), 7, dtype=torch.uint8, device="cuda"))
        if self.kind == "basic":
            out["near_ag"] = torch.full((K, B, self.L), -1, dtype=torch.int32, device="cuda")
        p = lambda t: None if t is None else t.data_ptr()
        rc = load().fg64_rollout_scenario(self.params, self.scenario, self.options, B, N, K, do_physics, obs_every, self.stage,
                                          p(self.px), p(self.py), p(self.vx), p(self.vy), p(acts), p(self.lm), p(self.opos),
                                          p(self.ovel), p(self.step_count), p(out["obs"]), p(out["reward"]), p(out["indiv"]),
                                          p(out["done"]), p(out.get("near_ag")), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, {k: v.cpu().numpy() for k, v in out.items()}

    def rollout(self, acts, obs_every=1):
        rc, out = self.launch(acts, obs_every)
        assert rc == 0, "fg64_rollout_scenario returned %d" % rc
        return out

    def step(self, act):
        return {k: v[0] for k, v in self.rollout(np.asarray(act)[None]).items()}

    def state(self):
        """dict(pos, vel [B,N,2], obst_pos, obst_vel [B,M,2] or None, step [B]) as the device holds them now"""
        st = lambda a, b: None if a is None else torch.stack((a, b), -1).cpu().numpy()
        return dict(pos=st(self.px, self.py), vel=st(self.vx, self.vy), obst_pos=None if self.opos is None else self.opos.cpu().numpy(),
                    obst_vel=None if self.ovel is None else self.ovel.cpu().numpy(), step=self.step_count.cpu().numpy())


def rollout64(g, params=None):
    """The fixture's T steps in ONE launch of the fp64 build of the PIPELINED rollout kernel (fg64_rollout_hd: rollout_kernel<9 | 27,
    ...> with real = double), free-running from the fixture's initial state.  Returns dict(pos, vel [B,N,2] after the launch;
    obs [T,B,N,6N], reward, indiv [T,B,N], done [T,B,N])."""
    acts = np.ascontiguousarray(np.asarray(g["acts"], dtype=np.float64))                # [T,B,N,2], fp32-representable values
    T, B, N = acts.shape[:3]
    env = Env64(g["pos0"], g["vel0"], g["ideal_shape"], g["ideal_vel"], indices=False)
    f = dict(dtype=torch.float64, device="cuda")
    act = torch.as_tensor(acts, **f)
    obs = torch.full((T, B, N, 6 * N), float("nan"), **f)
    rew = torch.full((T, B, N), float("nan"), **f)
    indiv = torch.full((T, B, N), float("nan"), **f)
    done = torch.full((T, B, N), 7, dtype=torch.uint8, device="cuda")
    rc = load().fg64_rollout_hd(params or env.params, B, N, T, env.px.data_ptr(), env.py.data_ptr(), env.vx.data_ptr(), env.vy.data_ptr(),
                                act.data_ptr(), env.shape.data_ptr(), env.ivel.data_ptr(), env.step_count.data_ptr(),
                                obs.data_ptr(), rew.data_ptr(), indiv.data_ptr(), done.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, "fg64_rollout_hd returned %d" % rc
    torch.cuda.synchronize()
    return dict(pos=env.pos(), vel=env.vel(), obs=obs.cpu().numpy(), reward=rew.cpu().numpy(), indiv=indiv.cpu().numpy(),
                done=done.cpu().numpy(), step=env.step_count.cpu().numpy())


def returns64(pos, vel, ideal_shape, ideal_vel, step, acts, gamma, params=None):
    """ONE launch of the fp64 build of returns_kernel (fg64_rollout_hd_returns: the product's geometry per agent count) over the
    candidates acts [C,K,B,N,2] from the state pos, vel [B,N,2], ideal_shape [B,N,2], ideal_vel [B,2], step [B].  The outputs are
    filled with NaN / -1 before the launch.  Returns dict(ret, indiv [C,B,N] float64, steps [B] int32)."""
    f = dict(dtype=torch.float64, device="cuda")
    acts = np.ascontiguousarray(np.asarray(acts, dtype=np.float64))
    C, K, B, N = acts.shape[:4]
    assert acts.shape == (C, K, B, N, 2)
    env = Env64(pos, vel, ideal_shape, ideal_vel, step=step, params=params, indices=False)
    assert (env.B, env.N) == (B, N)
    act = torch.as_tensor(acts, **f)
    ret = torch.full((C, B, N), float("nan"), **f)
    indiv = torch.full((C, B, N), float("nan"), **f)
    steps = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    rc = load().fg64_rollout_hd_returns(env.params, B, N, K, C, float(gamma), env.px.data_ptr(), env.py.data_ptr(),
                                        env.vx.data_ptr(), env.vy.data_ptr(), env.shape.data_ptr(), env.ivel.data_ptr(),
                                        env.step_count.data_ptr(), act.data_ptr(), ret.data_ptr(), indiv.data_ptr(),
                                        steps.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, "fg64_rollout_hd_returns returned %d" % rc
    torch.cuda.synchronize()
    return dict(ret=ret.cpu().numpy(), indiv=indiv.cpu().numpy(), steps=steps.cpu().numpy())
