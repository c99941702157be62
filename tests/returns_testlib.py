"""Helpers the `rollout_returns` tests share (tests/test_returns_cpu.py, tests/test_gpu_returns.py): the crowded start state and
the episode phases - functions of a seed, made with torch on the CPU, so that the CPU test can hold the GPU tests' inputs to
their conditions - the env, the candidate tensors, and the reference.  A plain module: no fixtures, nothing registered with pytest.

The reference is written here from `env.rollout`'s outputs alone: per candidate, restore the state, `rollout(a[c], out=...)` with
`auto_reset` off, then the recurrence as a Python loop over k of torch fp32 ops.  It calls neither `rollout_returns` nor the
returns kernel, so the fused launch and the replay route are both held to something independent.

`oracle_returns` is the second reference, in float64 and NumPy alone: the fp64 oracle (oracle/formation_oracle.py) stepped K times
per candidate, the discounted sum and the counting rule written out here.  It shares no code with the kernel or with `reference`;
the fp64 build of returns_kernel (tests/test_gpu_f64_returns.py) and the fp32 product are held to it, and tests/test_returns_cpu.py
holds it to the golden fixtures first."""
import numpy as np
import torch

import formation_gym
from oracle import formation_oracle as O

DEV = "cuda:0"
DIST_MIN = 0.06                     # formation_hd_env / basic_formation_env: 2 x agent.size (0.03)
FUSED_N = (3, 4, 8, 9, 16, 25, 27, 32)
SEED = 12                           # of the states and candidates of every GPU test: chosen so that the crowded states hold
                                    # contacts (tests/test_returns_cpu.py), env 0 - the single env of the B = 1 cases - included


def crowded_state(B, N, seed=SEED):
    """(pos, vel) [B, N, 2] fp32 on the CPU: the agents of every env inside a square of half-width 0.05 sqrt(N) - 3 agents within
    0.17, 32 within 0.57 - so that soft contacts (pairs closer than DIST_MIN) and collision penalties are part of every step,
    with velocities of a few tenths."""
    g = torch.Generator().manual_seed(1000 * seed + N)
    half = 0.05 * float(np.sqrt(N))
    pos = (torch.rand((B, N, 2), generator=g) * 2 - 1) * half
    vel = (torch.rand((B, N, 2), generator=g) * 2 - 1) * 0.3
    return pos, vel


def envs_in_contact(pos, dist_min=DIST_MIN):
    """bool [B]: the env has a pair of agents closer than `dist_min`."""
    d = (pos[:, :, None, :] - pos[:, None, :, :]).norm(dim=-1)
    d = d + torch.eye(pos.shape[1]) * 1e9
    return d.flatten(1).min(1).values < dist_min


def phases(B, K, world_length):
    """int32 [B] step counters: env 0 ends its episode at step 2 of a K-step launch, env 1 at step K exactly, env 2 is already
    past `world_length`, envs 3 and 4 are far from the end; further envs repeat the five."""
    five = [world_length - 2, world_length - K, world_length + 3, 0, 37]
    return torch.tensor([five[b % 5] for b in range(B)], dtype=torch.int32)


def expected_steps(step_count, K, world_length):
    """The issue's formula: min(K, max(1, world_length - step_count))."""
    return torch.clamp(world_length - step_count.to(torch.int64), min=1, max=K).to(torch.int32)


def env(N, B, K, name="formation_hd_env", seed=SEED, **kw):
    """`name` with N agents and B envs on the GPU, seeded and reset, then put into the crowded state at mixed episode phases."""
    e = formation_gym.make_env(name, False, N, num_envs=B, device=DEV, **kw)
    e.seed(seed)
    e.reset()
    pos, vel = crowded_state(B, N, seed)
    e.world.set_state(pos, vel)
    e.world.step_count.copy_(phases(B, K, int(e.world.world_length)))
    return e


def candidates_cpu(C, K, B, N, seed=SEED, mode=None):
    """Candidate actions [C, K, B, N, 2] fp32 in [-1, 1) on the CPU; mode 'index': [C, K, B, N] int32 indices 0 ... 4."""
    g = torch.Generator().manual_seed(7000 * seed + 100 * C + K)
    if mode == "index":
        return torch.randint(0, 5, (C, K, B, N), generator=g, dtype=torch.int32)
    return torch.rand((C, K, B, N, 2), generator=g) * 2 - 1


def candidates(C, K, B, N, seed=SEED, mode=None):
    """`candidates_cpu` on the GPU."""
    return candidates_cpu(C, K, B, N, seed, mode).to(DEV)


def env_facts(e):
    """Everything `rollout_returns` must leave alone, cloned: the state tensors, step counters, ideal shape / velocity (or the
    landmarks), the RNG offset and device counter, current_step, world_step, auto_reset."""
    w, sc = e.world, e.scenario
    tensors = {k: getattr(w, k).clone() for k in ("pos_x", "pos_y", "vel_x", "vel_y", "step_count", "landmark_pos")
               if torch.is_tensor(getattr(w, k, None))}
    tensors.update({k: getattr(sc, k).clone() for k in ("ideal_shape", "ideal_vel") if torch.is_tensor(getattr(sc, k, None))})
    if w.rng_counter is not None:
        tensors["rng_counter"] = w.rng_counter.clone()
    return tensors, (e._rng_offset, e.current_step, w.world_step, e.auto_reset)


def assert_same_facts(before, after):
    assert before[1] == after[1], (before[1], after[1])
    assert before[0].keys() == after[0].keys()
    for k in before[0]:
        assert torch.equal(before[0][k], after[0][k]), k


def reference(e, a, gamma):
    """(shared returns [C, B, N], individual returns [C, B, N], steps [B] int32) of candidates `a` from e's current state, by
    `env.rollout` and a Python loop (module docstring).  Leaves `e` as it found it."""
    C, K = int(a.shape[0]), int(a.shape[1])
    B, N, D = e.num_envs, e.num_agents, e._out["obs"].shape[-1]
    f = dict(dtype=torch.float32, device=DEV)
    g = torch.tensor(gamma, **f)
    shared, own = torch.empty((C, B, N), **f), torch.empty((C, B, N), **f)
    steps = None
    snap, auto_reset = e._snapshot(), e.auto_reset
    e.auto_reset = False
    try:
        for c in range(C):
            e._restore(snap)
            out = dict(obs=torch.empty((K, B, N, D), **f), reward=torch.empty((K, B, N), **f), indiv=torch.empty((K, B, N), **f),
                       done=torch.zeros((K, B, N), dtype=torch.uint8, device=DEV))
            e.rollout(a[c], out=out)
            done = out["done"][:, :, 0] != 0                              # [K, B]
            live = torch.ones((B,), dtype=torch.bool, device=DEV)          # no earlier step of the launch has set the done flag
            d = torch.ones((), **f)
            r_sh, r_own = torch.zeros((B, N), **f), torch.zeros((B, N), **f)
            n = torch.zeros((B,), dtype=torch.int32, device=DEV)
            for k in range(K):
                t_sh = d * out["reward"][k]                                # each product and each sum an op of its own
                t_own = d * out["indiv"][k]
                r_sh = torch.where(live[:, None], r_sh + t_sh, r_sh)
                r_own = torch.where(live[:, None], r_own + t_own, r_own)
                n = n + live.to(torch.int32)
                live = live & ~done[k]
                d = d * g
            shared[c], own[c] = r_sh, r_own
            if steps is None:
                steps = n
            else:
                assert torch.equal(steps, n)                                # the counted steps do not depend on the candidate
    finally:
        e._restore(snap)
        e.auto_reset = auto_reset
    return shared, own, steps


# ---- the fp64 reference: NumPy and the oracle, nothing of the kernel, of torch or of the device ----
def oracle_returns(state, acts, gamma, P=None):
    """(shared [C,B,N], indiv [C,B,N], steps [B] int32, margin [C,B]) in float64: the discounted returns of the candidates
    acts [C,K,B,N,2], each from a copy of `state` = dict(pos, vel [B,N,2], ideal_shape [B,N,2], ideal_vel [B,2], step [B]), by K
    calls of O.step_hd and R += d r, d *= gamma.  A step counts while no earlier step of the call has reached P.world_length -
    written out below from state["step"] alone; the oracle's done output is not looked at.  margin: the smallest cnt_margin of
    the pair's counted steps - how far the integer collision count, the one discontinuous term of the reward, is from flipping."""
    P = P or O.HdParams()
    acts = np.asarray(acts, dtype=np.float64)
    C, K, B, N = acts.shape[:4]
    assert acts.shape == (C, K, B, N, 2)
    steps = np.zeros(B, dtype=np.int32)
    for b in range(B):
        t = int(state["step"][b])
        for k in range(K):
            steps[b] += 1                                   # step k counts: none before it has reached the episode's end
            t += 1
            if t >= int(P.world_length):
                break
    shared, indiv = np.zeros((C, B, N)), np.zeros((C, B, N))
    margin = np.full((C, B), np.inf)
    for c in range(C):
        st = {k: np.array(v, dtype=np.int32 if k == "step" else np.float64) for k, v in state.items()}
        d = 1.0
        for k in range(K):
            st, out = O.step_hd(st, acts[c, k], P)
            live = k < steps                                 # [B]
            shared[c] += np.where(live[:, None], d * out["shared"][:, None], 0.0)
            indiv[c] += np.where(live[:, None], d * out["indiv"], 0.0)
            margin[c] = np.where(live, np.minimum(margin[c], out["cnt_margin"]), margin[c])
            d *= gamma
    return shared, indiv, steps, margin


def fixture_state(g):
    """The initial state of a golden fixture in the multi-env layout, as `oracle_returns` and f64_parity.returns64 take it"""
    B = g["pos0"].shape[0]
    return dict(pos=g["pos0"], vel=g["vel0"], ideal_shape=g["ideal_shape"], ideal_vel=g["ideal_vel"], step=np.zeros(B, dtype=np.int32))


def fixture_params(name, g):
    """The oracle's parameter object of a fixture that carries its own World constants (hd_n*_constants), else None"""
    from tests import option_cases
    return option_cases.fixture_case(name, g)["P"] if "world_dt" in g else None


def fixture_sums(g):
    """(steps [B], shared [B,N], indiv [B,N]): the steps up to and including the first recorded done flag, and the plain sums of
    the reference's recorded rewards over them"""
    T = g["acts"].shape[0]
    done = np.asarray(g["done"], dtype=bool)[:, :, 0]                         # [T,B]
    steps = np.where(done.any(0), done.argmax(0) + 1, T).astype(np.int32)
    live = (np.arange(T)[:, None] < steps[None, :])[..., None]
    shared = g["shared"] if g["shared"].ndim == 3 else np.repeat(g["shared"][..., None], g["acts"].shape[2], -1)
    return steps, (shared * live).sum(0), (g["indiv"] * live).sum(0)


def oracle_state(B, N, K, world_length=100, seed=SEED):
    """The GPU tests' crowded state at the mixed episode phases, in float64 for the oracle: `crowded_state` and `phases`
    (fp32-representable values), the ideal shape and velocity of O.reset_hd at the seeds seed + 1000 b."""
    pos, vel = crowded_state(B, N, seed)
    st = O.reset_hd(seed + 1000 * np.arange(B), N)
    return dict(pos=pos.double().numpy(), vel=vel.double().numpy(), ideal_shape=st["ideal_shape"], ideal_vel=st["ideal_vel"],
                step=phases(B, K, world_length).numpy())


def oracle_state_of(e):
    """The current state of a formation_hd_env as `oracle_returns` takes it: the env's fp32 values, exactly, in float64"""
    pos, vel = e.world.get_state()
    f = lambda t: t.double().cpu().numpy()
    return dict(pos=f(pos), vel=f(vel), ideal_shape=f(e.scenario.ideal_shape), ideal_vel=f(e.scenario.ideal_vel),
                step=e.world.step_count.cpu().numpy().astype(np.int32))


def oracle_candidates(C, K, B, N, seed=SEED):
    """`candidates_cpu` in float64 (fp32-representable values)."""
    return candidates_cpu(C, K, B, N, seed).double().numpy()


# The shapes the fp64 kernel is run at (tests/test_gpu_f64_returns.py; tests/test_returns_cpu.py holds the reference's mutants and
# margins on them): (N, B, C, K).  Every agent count at B = 5, C = 7 and an odd K = 7; at 3 and 27 agents (64 and 8 pairs per
# workgroup) K = 1, 2, 3 - no prefetch, a clamped second fetch, an unpaired last step -, one pair more than a workgroup, and at 3
# agents C = 32: env 2 (one counted step) owns pairs 64 ... 95, two whole waves of the second workgroup, which leave the loop
# after the first iteration beside waves that run all K.
F64_K = 7
F64_MAIN = [(N, 5, 7, F64_K) for N in FUSED_N]
F64_EDGES = [(N, 5, 7, k) for N in (3, 27) for k in (1, 2, 3)] + [(3, 5, 13, F64_K), (27, 5, 5, F64_K), (3, 5, 32, F64_K)]
F64_GAMMAS = (0.0, 0.5, 1.0)
F64_BOUND = 1e-9                    # x max(1, |R|): the pipelined rollout's free-run bound (per-step errors <= 7e-12, <= 25 steps)
# The fp32 product against the fp64 oracle (tests/test_gpu_returns.py: K = 3, gamma = 0.97, pairs with margin > F32_MARGIN), relative
# to max(1, |R|): twice the largest error measured over the eight agent counts (profiles/returns_parity.md), rounded up to one
# significant digit: measured 9.4e-8 ... 1.38e-7 (3 agents), two fp32 roundings of a return.  The widest tolerance any test of
# the returns uses: the mutants of tests/test_returns_cpu.py clear 100 x this.
F32_ORACLE_BOUND = 3e-7
F32_MARGIN = 1e-4
