"""Helpers the `rollout_returns` tests share (tests/test_returns_cpu.py, tests/test_gpu_returns.py): the crowded start state and
the episode phases - functions of a seed, made with torch on the CPU, so that the CPU test can hold the GPU tests' inputs to
their conditions - the env, the candidate tensors, and the reference.  A plain module: no fixtures, nothing registered with pytest.

The reference is written here from `env.rollout`'s outputs alone: per candidate, restore the state, `rollout(a[c], out=...)` with
`auto_reset` off, then the recurrence as a Python loop over k of torch fp32 ops.  It calls neither `rollout_returns` nor the
returns kernel, so the fused launch and the replay route are both held to something independent."""
import numpy as np
import torch

import formation_gym

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


def candidates(C, K, B, N, seed=SEED, mode=None):
    """Candidate actions [C, K, B, N, 2] in [-1, 1) on the GPU; mode 'index': [C, K, B, N] int32 indices 0 ... 4."""
    g = torch.Generator().manual_seed(7000 * seed + 100 * C + K)
    if mode == "index":
        return torch.randint(0, 5, (C, K, B, N), generator=g, dtype=torch.int32).to(DEV)
    return (torch.rand((C, K, B, N, 2), generator=g) * 2 - 1).to(DEV)


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
