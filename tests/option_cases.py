"""The inputs on which the World-option half of the step kernel (step_kernel<..., OPTS = true>) is checked in fp64, in the form
the fp64 oracle takes them - shared by the GPU tests (tests/test_gpu_f64_options.py), their CPU companion
(tests/test_f64_option_inputs.py) and profiles/parity_errors.py.  numpy and the oracle only.

  fixture_case(name, g)   one of the reference's option fixtures as dict(g, P, opts, comm): `g` in the multi-env layout of the
                          hd_* fixtures ([T,B,...] arrays, obs_t<k>), `opts` the keyword arguments of O.step_hd, `comm` [T,B,N,2]
  seeded_case(N, B)       a seeded oracle case at another agent count: random per-agent table, two hard walls and a soft one,
                          env 0 arranged so that every option branch is taken whatever N is
  oracle_free_run(...)    the oracle free-running over a case"""
import numpy as np

from oracle import formation_oracle as O

OPTION_FIXTURES = ["hd_n9_options", "hd_n27_walls", "hd_n9_masses", "hd_n27_masses", "hd_n9_flags", "hd_n6_immovable",
                   "hd_n5_comm", "hd_n6_scripted", "hd_n9_constants", "hd_n27_constants"]
SINGLE_ENV = ("hd_n6_immovable", "hd_n5_comm", "hd_n6_scripted")
ALL_WALLS = O.GOLDEN_WALLS + [w + (False,) for w in O.GOLDEN_SOFT_WALLS]

SEEDED_SHAPES = [(5, 9), (17, 5), (33, 3), (65, 2), (130, 2), (600, 1)]
SEEDED_STEPS = 6
# Seed and crowd scale (positions drawn in +-scale) of every shape, picked on the CPU from the oracle alone: contacts and wall
# forces in every case, and a crowd in which ONE rounding of the initial positions (x (1 + 1e-16 N(0,1))) moves nothing by more
# than 2e-12 within the six steps (tests/test_f64_option_inputs.py).  Masses of 0.5 ... 4 make contacts up to 16 times stiffer
# than the reference's unit masses (a light agent against a heavy one gains m_j / m_i^2), and at the density of the small cases
# 130 or 600 such agents amplify that one rounding to 1e-10 ... 3e-9 - which would measure the crowd, not the kernel.
SEEDED_SEEDS = {(5, 9): 7005, (17, 5): 7017, (33, 3): 7033, (65, 2): 7067, (130, 2): 7130, (600, 1): 7601}
SEEDED_SCALE = {5: 0.4, 17: 0.4, 33: 0.4, 65: 0.6, 130: 1.6, 600: 4.0}
# two hard walls and a soft one inside the crowd of seeded_case (positions within +-0.4 or wider)
SEEDED_WALLS = [("V", 0.25, (-0.2, 0.2), 0.04), ("H", -0.3, (-0.3, 0.1), 0.06), ("H", 0.26, (0.0, 0.4), 0.05, False)]


def _params(g=None, agent_size=None):
    P = O.HdParams()
    if g is not None and "world_dt" in g:
        P.dt = float(g["world_dt"]); P.damping = float(g["world_damping"])
        P.contact_force = float(g["world_contact_force"]); P.contact_margin = float(g["world_contact_margin"])
        P.mass = float(g["world_mass"]); P.agent_size = float(g["world_size"]); P.world_length = int(g["world_world_length"])
    if agent_size is not None:
        P.agent_size = float(agent_size)
    return P


def _hetero(g):
    return dict(mass=g["agent_mass"], size=g["agent_size"], accel=g["agent_accel"], max_speed=g["agent_max_speed"])


def fixture_case(name, g):
    """dict(g, P, opts, comm) of an option fixture.  The three single-env fixtures (driven through core.py's World API, which
    records positions, velocities, individual rewards and every step's observation) are put into the [T, B = 1, ...] layout of
    the others; what that API does not record follows from what it does: shared reward = the sum of the recorded individual
    rewards (environment.py:136), done = step >= world_length (:172-178), and the index assignments with their tie margins and
    the collision-count margin are the oracle's on the REFERENCE's recorded state."""
    P, opts, comm = _params(g), {}, None
    if name == "hd_n9_options":
        opts = dict(max_speed=0.6, accel=3.0, walls=O.GOLDEN_WALLS)
    elif name == "hd_n27_walls":
        opts = dict(walls=O.GOLDEN_WALLS)
    elif name == "hd_n9_masses":
        opts = _hetero(g)
    elif name == "hd_n27_masses":
        opts = dict(_hetero(g), walls=O.GOLDEN_WALLS)
    elif name == "hd_n9_flags":
        opts = dict(_hetero(g), walls=ALL_WALLS, collide=g["agent_collide"], ghost=g["agent_ghost"])
        P = _params(g, g["agent_size"][0])
    elif name == "hd_n6_immovable":
        opts = dict(mass=g["mass"], movable=g["movable"], collide=g["collide"])
    elif name == "hd_n6_scripted":
        opts = dict(mass=g["mass"], scripted=g["scripted"])
    if name not in SINGLE_ENV:
        return dict(name=name, g=g, P=P, opts=opts, comm=None)
    T, N = g["acts"].shape[:2]
    acts = np.array(g["acts"], dtype=np.float64)
    if name == "hd_n6_scripted":
        acts[:, g["scripted"]] = g["u_scripted"]                 # the callback's action.u, as the reference computed it
    if name == "hd_n5_comm":
        comm = np.asarray(g["c"], dtype=np.float64)[:, None]
    m = dict(acts=acts[:, None], pos0=g["pos0"][None], vel0=g["vel0"][None], ideal_shape=g["ideal_shape"][None],
             ideal_vel=g["ideal_vel"][None], pos=g["pos"][:, None], vel=g["vel"][:, None], indiv=g["indiv"][:, None],
             obs_steps=np.arange(1, T + 1))
    m["shared"] = np.repeat(m["indiv"].sum(-1, keepdims=True), N, -1)
    m["done"] = np.repeat((np.arange(1, T + 1) >= P.world_length)[:, None, None], N, -1)
    per_step = [O.reward_hd(m["pos"][t], m["vel"][t], m["ideal_shape"], m["ideal_vel"], P, size=opts.get("size"),
                            collide=opts.get("collide")) for t in range(T)]
    for k in ("near_lm", "near_ag", "gap_lm", "gap_ag", "cnt_margin", "cnt"):
        m[k] = np.stack([r[k] for r in per_step])
    for t in range(T):
        m["obs_t%d" % (t + 1)] = g["obs"][t][None]
    return dict(name=name, g=m, P=P, opts=opts, comm=comm)


def seeded_case(N, B, steps=SEEDED_STEPS, seed=None):
    """A crowded random case of N agents (positions scaled by SEEDED_SCALE, random initial velocities) with a per-agent table - masses
    0.5 ... 4, sizes 0.02 ... 0.06, accel / max_speed on about half the agents, agent 2 immovable, agent 4 non-colliding, agent 1 a
    ghost - among SEEDED_WALLS.  Env 0 puts agents 0 ... 4 where each option branch is taken in the first step whatever N is:
      agent 0  past the end of the vertical wall by half its size, inside its contact distance (corner rounding), in contact with
      agent 1  a ghost of another mass (mass ratio) that sits inside the soft wall (soft-wall pass-through);
      agent 3  (mass 4) overlaps the immovable agent 2 (mass 0.5): the immovable-partner rule; and
      agent 4  non-colliding, 0.045 from agent 3: inside their contact distance (0.12) and their own penalty distance
               (0.5 * 0.12) but outside the uniform one (0.03).
    Speed clamps and accel gains act on the randomly chosen agents from 5 up and, in envs 1 ..., on all of them.
    Returns dict(state, acts [steps,B,N,2] (fp32-representable), P, opts)."""
    rs = np.random.RandomState(SEEDED_SEEDS[(N, B)] if seed is None else seed)
    st = O.reset_hd(rs.randint(0, 100000, B), N)
    st["pos"] *= SEEDED_SCALE[N]
    st["vel"] = rs.uniform(-0.5, 0.5, (B, N, 2))
    acts = rs.uniform(-1, 1, (steps, B, N, 2)).astype(np.float32).astype(np.float64)
    mass = rs.uniform(0.5, 4.0, N); size = rs.uniform(0.02, 0.06, N)
    accel = np.where(rs.rand(N) < 0.5, rs.uniform(1.5, 4.0, N), np.nan)
    max_speed = np.where(rs.rand(N) < 0.5, rs.uniform(0.15, 0.4, N), np.nan)
    mass[:5] = [3.0, 0.7, 0.5, 4.0, 1.5]
    size[:5] = [0.03, 0.03, 0.04, 0.06, 0.06]
    accel[:5] = [np.nan, 2.0, np.nan, np.nan, 3.0]
    max_speed[:5] = [np.nan, np.nan, 0.2, np.nan, 0.3]
    movable = np.ones(N, dtype=bool); movable[2] = False
    collide = np.ones(N, dtype=bool); collide[4] = False
    ghost = np.zeros(N, dtype=bool); ghost[1] = True
    p = st["pos"][0]
    p[0] = (0.28, 0.215)
    p[1] = (0.23, 0.245)
    p[2] = (-0.2, -0.05)
    p[3] = (-0.2 + 0.09, -0.05)
    p[4] = (-0.2 + 0.09, -0.05 + 0.045)
    # nobody else of env 0 inside the arranged spots
    for j in range(5, N):
        while min(np.hypot(*(p[j] - p[k])) for k in range(5)) < 0.15:
            p[j] = rs.uniform(-0.4, 0.4, 2)
    st["vel"][0, :5] = 0.0
    acts[0, 0, :5] = 0.0
    opts = dict(mass=mass, size=size, accel=accel, max_speed=max_speed, movable=movable, collide=collide, ghost=ghost,
                walls=SEEDED_WALLS)
    return dict(state=st, acts=acts, P=O.HdParams(), opts=opts)


def wall_hits(pos, P, opts):
    """entities of [B,N,2] on which some wall of `opts` exerts a force"""
    N = pos.shape[1]
    sz = np.full(N, P.agent_size) if opts.get("size") is None else np.asarray(opts["size"], dtype=np.float64)
    hit = np.zeros(pos.shape[:2], dtype=bool)
    for w in opts.get("walls") or []:
        hit |= (O.wall_force(pos, sz[None, :], w, P, ghost=opts.get("ghost")) != 0).any(-1)
    return hit


def oracle_free_run(state, acts, P, opts, comm=None, blind=(), drop=()):
    """The fp64 oracle free-running from `state` over acts [T,B,N,2].  `blind` names branches of O.BLINDABLE to leave out,
    `drop` the options to withhold altogether.  Returns [T, ...] arrays of pos, vel, indiv, shared, cnt, cnt_margin, obs and the
    number of (step, entity) pairs with a wall force."""
    o = {k: v for k, v in opts.items() if k not in drop}
    if blind:
        o["blind"] = tuple(blind)
    st = dict(state, step=np.array(state["step"]))
    out = dict(pos=[], vel=[], indiv=[], shared=[], cnt=[], cnt_margin=[], obs=[])
    hits = 0
    for t in range(acts.shape[0]):
        hits += int(wall_hits(st["pos"], P, o).sum())
        kw = dict(o) if comm is None else dict(o, comm=comm[t])
        st, r = O.step_hd(st, acts[t], P, **kw)
        out["pos"].append(st["pos"]); out["vel"].append(st["vel"])
        for k in ("indiv", "shared", "cnt", "cnt_margin", "obs"):
            out[k].append(r[k])
    res = {k: np.stack(v) for k, v in out.items()}
    res["wall_hits"] = hits
    return res


def fixture_state(c):
    g = c["g"]
    B = g["pos0"].shape[0]
    return dict(pos=g["pos0"], vel=g["vel0"], ideal_shape=g["ideal_shape"], ideal_vel=g["ideal_vel"], step=np.zeros(B, dtype=np.int32))
