"""The inputs on which the run-time-count kernel of the landmark scenarios (fg::scn_kernel) is checked in fp64, in the form the
fp64 oracle takes them - shared by the GPU tests (tests/test_gpu_f64_scenarios.py), their CPU companion
(tests/test_f64_scenario_inputs.py) and profiles/f64_scenarios.py.  numpy and the oracle only.

  fixture_case(name, g)    one of the reference's 14 landmark fixtures as dict(kind, P, opts, state, acts, ref)
  seeded_case(i)           SEEDED[i]: a seeded oracle case at another entity count (every lane-group width and workgroup size)
  floor_case(N)            obstacles straddling obstacle_floor with agents in contact with each
  oracle_free_run(...)     the oracle free-running over a case, optionally blind to one branch"""
import copy

import numpy as np

from oracle import formation_oracle as O

FIXTURES = [("basic_n3", "basic"), ("basic_n4_flags", "basic"), ("partial_n3", "partial"), ("partial_n5", "partial"),
            ("partial_n9_crowd", "partial"), ("partial_n6_masses", "partial"), ("partial_n6_immovable", "partial"),
            ("range_n4", "range"), ("range_n7_crowd", "range"), ("obst_n4", "obstacle"), ("obst_n8", "obstacle"),
            ("obst_n5_masses", "obstacle"), ("obst_n5_flags", "obstacle"), ("obst_n5_immovable", "obstacle")]
KIND_OF = dict(FIXTURES)
ALL_WALLS = O.GOLDEN_WALLS + [w + (False,) for w in O.GOLDEN_SOFT_WALLS]
WALLED = ("basic_n4_flags", "obst_n5_flags", "obst_n5_immovable", "partial_n6_immovable")    # as tests/test_oracle_golden.py runs them
OPTION_KEYS = ("mass", "size", "max_speed", "movable", "collide", "ghost")


def params(kind, **over):
    """The oracle's parameter object of a scenario kind, with attributes replaced (how a branch is blinded: obs_range = inf ...)"""
    P = O.BasicParams() if kind == "basic" else O.ScnParams(kind)
    for k, v in over.items():
        setattr(P, k, v)
    return P


def fixture_case(name, g):
    """dict(name, kind, P, opts, state, acts [T,B,N,2], ref) of a landmark fixture.  opts: the keyword arguments of O.step_scn /
    O.step_basic (per-agent table, flags, walls).  ref: pos, vel [T,B,N,2], obs [T,B,N,D], indiv [T,B,N]; opos, ovel [T,B,M,2]
    (obstacle); shared, done [T,B,N] where the fixture recorded them (the two *_immovable fixtures, driven through core.py's World
    API, did not)."""
    kind = KIND_OF[name]
    P = params(kind)
    L = P.num_landmarks
    opts = {k: np.asarray(g["agent_" + k]) for k in OPTION_KEYS if "agent_" + k in g and np.ndim(g["agent_" + k]) == 1}
    if "max_speed" in opts and np.isnan(opts["max_speed"]).all():
        del opts["max_speed"]
    if name in WALLED:
        opts["walls"] = ALL_WALLS
    B = g["pos0"].shape[0]
    lm0 = g["landmarks"] if "landmarks" in g else g["lm0"]
    state = dict(pos=np.array(g["pos0"], dtype=np.float64), vel=np.array(g["vel0"], dtype=np.float64),
                 landmarks=np.array(lm0[:, :L], dtype=np.float64), step=np.zeros(B, dtype=np.int32))
    ref = dict(pos=g["pos"], vel=g["vel"], obs=g["obs"], indiv=g["indiv"], shared=g["shared"] if "shared" in g else None,
               done=g["done"] if "done" in g else None, opos=None, ovel=None)
    if kind == "obstacle":
        state["obst_pos"] = np.array(g["lm0"][:, L:], dtype=np.float64)
        state["obst_vel"] = np.array(g["lmvel0"][:, L:], dtype=np.float64)
        ref["opos"] = g["lm"][:, :, L:]
        ref["ovel"] = g["lmvel"][:, :, L:]
    return dict(name=name, kind=kind, P=P, opts=opts, state=state, acts=np.asarray(g["acts"], dtype=np.float64), ref=ref)


def sizes_of(N, P, opts):
    return np.full(N, P.agent_size) if opts.get("size") is None else np.asarray(opts["size"], dtype=np.float64)


def threshold_margin(kind, pos, opos, P, opts):
    """[B]: how far the closest pair of an env is from its collision threshold - agent-agent |dist - (size_a + size_b)| (basic: the
    threshold of BasicParams is the same sum), agent-obstacle |dist - (size_a + obstacle_size)|.  Where it is below the bound of a
    comparison, the integer collision count (and so the rewards) of that env may differ legitimately."""
    N = pos.shape[1]
    sz = sizes_of(N, P, opts)
    PD = np.sqrt(((pos[:, :, None] - pos[:, None]) ** 2).sum(-1))
    m = (np.abs(PD - (sz[:, None] + sz[None, :])) + 10 * np.eye(N)).min((1, 2))
    if opos is not None and opos.shape[1]:
        OD = np.sqrt(((pos[:, :, None] - opos[:, None]) ** 2).sum(-1))
        m = np.minimum(m, np.abs(OD - (sz[None, :, None] + P.obstacle_size)).min((1, 2)))
    return m


def oracle_step(kind, state, act, P, opts):
    if kind == "basic":
        return O.step_basic(state, act, P, **opts)
    return O.step_scn(kind, state, act, P, **opts)


def _index_order_neighbours(kind, pos, vel, lm, P):
    """the observation of `partial` from an oracle blind to the ring: the first num_obs OTHER agents in index order"""
    N, L = pos.shape[1], lm.shape[1]
    full = O.observation_scn("range", pos, vel, lm, None, params("range", obs_range=np.inf))
    head = 2 + 2 * L
    out = np.zeros((pos.shape[0], N, head + 2 * P.num_obs + 2 * (N - 1)))
    out[:, :, :head] = full[:, :, :head]
    k = min(P.num_obs, N - 1)
    out[:, :, head:head + 2 * k] = full[:, :, head:head + 2 * k]
    return out


def oracle_free_run(kind, state, acts, P, opts, drop=(), blind=(), **over):
    """The fp64 oracle free-running from `state` over acts [T,B,N,2].  A branch is blinded by withholding options (`drop`), by
    replacing parameters (`over`: obs_range = inf, obstacle_floor = -inf ...), or - blind = ("ring",) / ("self",) - by restating
    the one output the branch decides from the oracle's own pieces.  Returns [T, ...] arrays: pos, vel, obs, indiv, shared, done,
    margin [T,B] (threshold_margin of the post-step state), and opos, ovel for the obstacle scenario."""
    o = {k: v for k, v in opts.items() if k not in drop}
    P = copy.copy(P)
    for k, v in over.items():
        setattr(P, k, v)
    st = dict(state, step=np.array(state["step"]))
    if kind in ("partial", "range"):                           # O.step_scn takes the (empty) obstacle arrays of every kind
        st["obst_pos"] = st["obst_vel"] = np.zeros((st["pos"].shape[0], 0, 2))
    keys = ("pos", "vel", "obs", "indiv", "shared", "done", "margin") + (("opos", "ovel") if kind == "obstacle" else ())
    out = {k: [] for k in keys}
    for t in range(acts.shape[0]):
        st, r = oracle_step(kind, st, acts[t], P, o)
        obs, indiv = r["obs"], r["indiv"]
        if "ring" in blind:
            obs = _index_order_neighbours(kind, st["pos"], st["vel"], st["landmarks"], P)
        if "self" in blind:                                   # basic_formation_env.py:49-51 without the agent itself
            counted = np.ones(indiv.shape[1], dtype=bool) if o.get("collide") is None else np.asarray(o["collide"], dtype=bool)
            indiv = indiv + counted[None, :]
        out["pos"].append(st["pos"]); out["vel"].append(st["vel"]); out["obs"].append(obs); out["indiv"].append(indiv)
        out["shared"].append(r["shared"]); out["done"].append(r["done"])
        out["margin"].append(threshold_margin(kind, st["pos"], st.get("obst_pos"), P, o))
        if kind == "obstacle":
            out["opos"].append(st["obst_pos"]); out["ovel"].append(st["obst_vel"])
    return {k: np.stack(v) for k, v in out.items()}


# ---------------------------------------------------------------------------
# seeded oracle cases: (kind, N, B, crowd, table).  N + M walks every lane-group width of scn_kernel (4, 8, 16, 32, 64 lanes per
# env in 64-thread workgroups) for every kind and every whole-workgroup size (128, 256, 512, 1024 threads); B leaves the last
# workgroup ragged (64 / G envs per workgroup); the staged image fits the fp64 build's 160 KB of LDS up to ~65 agents and not
# beyond; `table` = a per-agent table with every flag and a speed clamp, among walls.
# ---------------------------------------------------------------------------
SEEDED_STEPS = 6
SEEDED = [
    ("basic", 3, 33, 0.3, False), ("partial", 4, 19, 0.2, False), ("range", 3, 17, 0.3, False), ("obstacle", 1, 18, 0.5, False),
    ("basic", 5, 9, 0.5, False), ("partial", 7, 11, 0.2, False), ("range", 8, 13, 0.3, False), ("obstacle", 5, 10, 0.5, False),
    ("basic", 13, 5, 0.5, False), ("partial", 16, 7, 0.3, False), ("range", 13, 6, 0.3, False), ("obstacle", 13, 5, 0.5, False),
    ("basic", 30, 3, 0.5, False), ("partial", 30, 3, 0.5, False), ("range", 32, 5, 0.5, False), ("obstacle", 29, 3, 0.5, False),
    ("basic", 61, 3, 0.5, False), ("partial", 62, 2, 0.5, False), ("range", 64, 3, 0.5, False), ("obstacle", 61, 2, 0.5, False),
    ("basic", 65, 2, 0.5, False), ("partial", 65, 2, 0.5, False), ("range", 90, 2, 0.5, False), ("obstacle", 62, 3, 0.5, False),
    ("obstacle", 90, 2, 0.5, True), ("partial", 200, 2, 0.5, False), ("obstacle", 200, 2, 0.5, False),
    ("range", 500, 1, 0.5, False), ("basic", 500, 2, 0.5, False), ("partial", 1000, 1, 0.5, False), ("obstacle", 1000, 1, 0.5, False),
]
SEEDED_WALLS = [("V", 0.25, (-0.2, 0.2), 0.04), ("H", -0.3, (-0.3, 0.1), 0.06), ("H", 0.26, (0.0, 0.4), 0.05, False)]
FG64_LDS_LIMIT = 160 * 1024


def seeded_id(c):
    return "%s-n%d-b%d%s" % (c[0], c[1], c[2], "-table" if c[4] else "")


def seeded_scale(N, size, crowd):
    """Positions are drawn in +-scale: the crowd factor for a handful of agents, and from there a constant density (about one
    contact per three agents) - a thousand agents of radius 0.1 inside +-0.5 would be one lump whose stiffness amplifies a single
    rounding beyond any bound within six steps, which would measure the crowd and not the kernel."""
    return max(crowd, 2.5 * size * np.sqrt(N))


def geometry(kind, N, P):
    """(G, T, E, D) of scn_kernel for N agents: lanes per env, threads and envs per workgroup, observation width"""
    M = P.num_obstacles if kind == "obstacle" else 0
    G = 4
    while G < N + M:
        G *= 2
    nbr = P.num_obs if kind == "partial" else N - 1
    D = 2 + (2 if kind == "basic" else 0) + 2 * P.num_landmarks + 2 * M + 2 * nbr + 2 * (N - 1)
    return G, max(G, 64), (64 // G if G <= 64 else 1), D


def lds_bytes(kind, N, P, stage):
    """scn_lds_bytes (csrc/fg_scn_kernel.hpp) of the fp64 build: 16-byte table entries, 8-byte image values"""
    G, T, E, D = geometry(kind, N, P)
    M = P.num_obstacles if kind == "obstacle" else 0
    return (E * (2 * (N + M) + P.num_landmarks) + (32 if G > 64 else 0)) * 16 + (E * N * D * 8 if stage else 0)


def _table(rs, N, size):
    """every flag and a speed clamp: masses 0.5 ... 3, sizes 0.6 ... 1.4 of the scenario's, a clamp on half the agents; agent 0 a
    ghost, agent 2 immovable, agent 3 non-colliding"""
    mass = rs.uniform(0.5, 3.0, N); sz = size * rs.uniform(0.6, 1.4, N)
    max_speed = np.where(rs.rand(N) < 0.5, rs.uniform(0.15, 0.4, N), np.nan)
    mass[:5] = [0.7, 2.5, 0.5, 1.5, 0.6]; sz[:5] = size
    max_speed[:5] = [np.nan, 0.2, np.nan, np.nan, 0.3]
    movable = np.ones(N, dtype=bool); movable[2] = False
    collide = np.ones(N, dtype=bool); collide[3] = False
    ghost = np.zeros(N, dtype=bool); ghost[0] = True
    return dict(mass=mass, size=sz, max_speed=max_speed, movable=movable, collide=collide, ghost=ghost, walls=SEEDED_WALLS)


def seeded_case(i):
    """dict(kind, P, opts, state, acts [6,B,N,2] (fp32-representable values)) of SEEDED[i].  A `table` case arranges env 0 so that
    every flag decides something within the first steps: agent 0 (a ghost) sits inside the soft wall; agent 1 (mass 2.5) overlaps the
    immovable agent 2 (mass 0.5); the non-colliding agent 3 overlaps agent 4; the speed clamps act on agents 1, 4 and half the rest."""
    kind, N, B, crowd, table = SEEDED[i]
    rs = np.random.RandomState(8100 + i)
    P = params(kind)
    L = P.num_landmarks
    scale = seeded_scale(N, P.agent_size, crowd)
    state = dict(pos=rs.uniform(-1, 1, (B, N, 2)) * scale, vel=rs.uniform(-0.3, 0.3, (B, N, 2)),
                 landmarks=rs.uniform(-1, 1, (B, L, 2)), step=rs.randint(0, P.world_length - 8, B).astype(np.int32))
    if kind == "obstacle":
        M = P.num_obstacles
        state["obst_pos"] = rs.uniform(-0.8, 0.8, (B, M, 2)) * scale
        state["obst_vel"] = np.tile(np.array(P.obstacle_vel, dtype=np.float64), (B, M, 1))
    acts = rs.uniform(-1, 1, (SEEDED_STEPS, B, N, 2)).astype(np.float32).astype(np.float64)
    opts = {}
    if table:
        opts = _table(rs, N, P.agent_size)
        p = state["pos"][0]
        s = P.agent_size
        p[0] = (0.2, 0.26 + 0.3 * s)
        p[1] = (-0.6, -0.7); p[2] = (-0.6 + 1.5 * s, -0.7)
        p[3] = (0.7, -0.6); p[4] = (0.7, -0.6 + 1.2 * s)
        for j in range(5, N):                                  # nobody else of env 0 inside the arranged spots
            while min(np.hypot(*(p[j] - p[k])) for k in range(5)) < 4 * s:
                p[j] = rs.uniform(-1, 1, 2) * scale
        if kind == "obstacle":
            q = state["obst_pos"][0]
            for k in range(q.shape[0]):
                while min(np.hypot(*(q[k] - p[j])) for j in range(5)) < 4 * s:
                    q[k] = rs.uniform(-0.8, 0.8, 2) * scale
        state["vel"][0, :5] = 0.0
        acts[0, 0, :5] = 0.0
    return dict(name=seeded_id(SEEDED[i]), kind=kind, P=P, opts=opts, state=state, acts=acts)


# ---------------------------------------------------------------------------
# the obstacle floor (formation_hd_obs_env.py:84-89): no fixture reaches it (obstacles sink 0.075 per step from y >= 2, episodes
# last 50 steps, the floor is at -2.2)
# ---------------------------------------------------------------------------
FLOOR_SHAPES = [(4, 5), (70, 2)]          # (N, B): a lane-group env and a whole-workgroup env


def floor_case(N, B, steps=SEEDED_STEPS, table=False, seed=None):
    """The obstacle scenario with its three obstacles around obstacle_floor: obstacle 0 starts 0.05 ... 0.2 above the floor, falling
    (it crosses inside the launch: 0.1 per step), obstacle 1 below the floor with velocity 0, obstacle 2 far above.  Agents 0, 1, 2
    start within contact distance of obstacle 0, 1, 2 (agent 1 under its obstacle, so that the push lifts the stopped obstacle; the
    rest of the agents are drawn around the floor, away from the obstacles).  The obstacles are 1.2 apart."""
    rs = np.random.RandomState((8800 + N) if seed is None else seed)
    P = params("obstacle")
    L, M = P.num_landmarks, P.num_obstacles
    reach = P.agent_size + P.obstacle_size
    ob = np.zeros((B, M, 2))
    ob[:, :, 0] = np.array([-1.2, 0.0, 1.2])[None] + rs.uniform(-0.1, 0.1, (B, M))
    ob[:, 0, 1] = P.obstacle_floor + rs.uniform(0.05, 0.2, B)
    ob[:, 1, 1] = P.obstacle_floor - rs.uniform(0.005, 0.08, B)
    ob[:, 2, 1] = P.obstacle_floor + rs.uniform(1.5, 2.0, B)
    ov = np.tile(np.array(P.obstacle_vel, dtype=np.float64), (B, M, 1))
    ov[:, 1] = 0.0
    width = max(2.0, 2.5 * P.agent_size * np.sqrt(N))
    pos = np.stack((rs.uniform(-width, width, (B, N)), P.obstacle_floor + rs.uniform(0.6, 1.2, (B, N))), -1)
    ang = np.stack((rs.uniform(0.3, 2.8, B), rs.uniform(-2.2, -0.9, B), rs.uniform(0.3, 2.8, B)), 1)      # above, below, above
    for k in range(3):
        d = reach * (rs.uniform(0.6, 0.85, B) if k == 1 else rs.uniform(0.8, 0.97, B))      # the stopped one is pushed hard
        pos[:, k] = ob[:, k] + d[:, None] * np.stack((np.cos(ang[:, k]), np.sin(ang[:, k])), -1)
    for b in range(B):                                        # nobody else within reach of an obstacle at the start
        for j in range(3, N):
            while np.hypot(*(pos[b, j] - ob[b]).T).min() < 2 * reach or np.hypot(*(pos[b, j] - pos[b, :3]).T).min() < 3 * P.agent_size:
                pos[b, j] = (rs.uniform(-width, width), P.obstacle_floor + rs.uniform(0.6, 1.2))
    state = dict(pos=pos, vel=rs.uniform(-0.1, 0.1, (B, N, 2)), landmarks=rs.uniform(-1, 1, (B, L, 2)) + np.array([0.0, P.obstacle_floor + 1]),
                 obst_pos=ob, obst_vel=ov, step=np.zeros(B, dtype=np.int32))
    acts = rs.uniform(-1, 1, (steps, B, N, 2)).astype(np.float32).astype(np.float64)
    return dict(name="floor-n%d-b%d" % (N, B), kind="obstacle", P=P, opts={}, state=state, acts=acts)


def floor_states(case, run):
    """What the oracle's own run `run` of a floor case shows, per obstacle over the launch: dict of boolean [B, M]
      falling   above the floor after every step (velocity re-armed every time)
      crossing  above the floor at the start, below it at the end (velocity zeroed inside the launch)
      moved     below the floor from the start, yet its position changes: a stopped obstacle that contact pushes
      rearmed   below the floor from the start and lifted above it at some step (velocity re-armed from zero)"""
    floor = case["P"].obstacle_floor
    y0 = case["state"]["obst_pos"][..., 1]
    y = run["opos"][..., 1]
    below0 = y0 <= floor
    return dict(falling=(y0 > floor) & (y > floor).all(0), crossing=(y0 > floor) & (y[-1] <= floor),
                moved=below0 & (np.abs(run["opos"] - case["state"]["obst_pos"][None]).max((0, 3)) > 1e-3),
                rearmed=below0 & (y > floor).any(0))
