#!/usr/bin/env python3
"""Scoring C candidate action sequences of K steps from one state: `env.rollout_returns` against what the API offered before it.

  fused      env.rollout_returns(a, gamma) on the env of B envs: ONE returns_kernel launch (fg_rollout_hd_returns) that reads the
             state, runs C x B (candidate, env) pairs and stores two floats per agent and pair
  fused_again  the same variant a second time in the alternation: the difference of the two medians is the run-to-run spread
  baseline   a second env of C * B envs holding C copies of the state; env.rollout of the candidates regrouped to
             [K, C * B, N, 2] with obs_every = K into caller-owned buffers (a bound launch): every step's rewards and done
             flags and one observation block are written and then thrown away, and the discounted sums are not even formed.
             The regrouping and the state copy are NOT timed: the state is put back before every call, outside the events
  replay     env.rollout_returns through the replay route (snapshot, C x (restore, rollout), restore), first shape only

All envs start from the reset state with step counters 0 (no episode ends inside the K steps, so the fused launch runs all of
them, as the baseline does).  One process: every variant of a shape is built and warmed for a second, then the variants
ALTERNATE for ROUNDS rounds; a round's block is a run of calls, each between two device events, whose event times are summed
(at least a second of device time per block); a variant is reported as the median of its blocks with their min - max.
Usage:  python3 profiles/rollout_returns.py            (markdown on stdout)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-formation_amd")]

K = 20
GAMMA = 0.97
SHAPES = ((27, 4096, 8), (9, 4096, 16), (3, 16384, 16), (27, 1, 4096))      # (agents, envs, candidates)
ROUNDS = 5
BLOCK_MS = 1000.0


def bytes_per_step(N, C):
    """Bytes moved per (candidate, env, step), from the shapes: (fused, baseline)."""
    state = 6 * 4 * N + 12                                   # p, v, ideal shape per agent; ideal velocity and step counter
    fused = 8 * N + (state + 8 * N + 4.0 / C) / K            # the step's actions; per launch the state in, two returns out
    base = 8 * N + 9 * N + (state + 16 * N + 4 + 24 * N * N) / K   # actions, reward + indiv + done; state in and out, one obs block
    return fused, base


def shape(N, B, C, with_replay):
    import torch
    import formation_gym
    dev = "cuda:0"

    def make(nenv):
        e = formation_gym.make_env("formation_hd_env", False, N, num_envs=nenv, device=dev)
        e.seed(1)
        e.reset()
        return e
    env, big = make(B), make(C * B)
    torch.manual_seed(0)
    a = torch.rand((C, K, B, N, 2), device=dev) * 2 - 1
    # the baseline's inputs: candidate c of env b is env c B + b of the big env
    a_big = a.permute(1, 0, 2, 3, 4).reshape(K, C * B, N, 2).contiguous()
    w, sc = env.world, env.scenario
    state = {k: getattr(w, k).repeat(C, 1) for k in ("pos_x", "pos_y", "vel_x", "vel_y")}
    big.scenario.ideal_shape.copy_(sc.ideal_shape.repeat(C, 1, 1))
    big.scenario.ideal_vel.copy_(sc.ideal_vel.repeat(C, 1))
    f = dict(dtype=torch.float32, device=dev)
    out = dict(obs=torch.empty((1, C * B, N, 6 * N), **f), reward=torch.empty((K, C * B, N), **f),
               indiv=torch.empty((K, C * B, N), **f), done=torch.zeros((K, C * B, N), dtype=torch.uint8, device=dev))
    assert env.returns_path() == "fused"
    replay_env = None
    if with_replay:
        replay_env = make(B)
        replay_env._returns_replay_only = True
        assert replay_env.returns_path() == "replay"

    def put_back():
        for k, v in state.items():
            getattr(big.world, k).copy_(v)
        big.world.step_count.zero_()

    bodies = {"fused": (None, lambda: env.rollout_returns(a, GAMMA)),
              "baseline": (put_back, lambda: big.rollout(a_big, out=out, obs_every=K)),
              "fused_again": (None, lambda: env.rollout_returns(a, GAMMA))}
    if with_replay:
        bodies["replay"] = (None, lambda: replay_env.rollout_returns(a, GAMMA))

    # same results first: faster and different is not faster
    put_back()
    big.rollout(a_big, out=out, obs_every=K)
    d = GAMMA ** torch.arange(K, **f)
    ret, info = env.rollout_returns(a, GAMMA)
    ref = (out["reward"] * d[:, None, None]).sum(0).view(C, B, N)
    err = ((ret - ref).abs().max() / ref.abs().max()).item()
    assert err < 1e-5, err                                   # (the sums are associated differently: not the bits)

    def timed(prepare, call, reps):
        pairs = []
        for _ in range(reps):
            if prepare is not None:
                prepare()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            pairs.append((e0, e1))
        torch.cuda.synchronize()
        return sum(x.elapsed_time(y) for x, y in pairs)      # ms of device time between the events

    reps = {}
    for name, (prepare, call) in bodies.items():
        timed(prepare, call, 3)
        ms, n = 0.0, 0
        while ms < BLOCK_MS:                                  # warm: a second of it, and the call's own time
            ms += timed(prepare, call, 4); n += 4
        reps[name] = max(4, int(n * BLOCK_MS / ms) + 1)
    blocks = {name: [] for name in bodies}
    for _ in range(ROUNDS):
        for name, (prepare, call) in bodies.items():         # the variants alternate
            blocks[name].append(timed(prepare, call, reps[name]) / reps[name] * 1e6 / (C * B * K))   # ns per (candidate, env, step)
    return {name: (statistics.median(v), min(v), max(v)) for name, v in blocks.items()}, err


def main():
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("ns (1e-3 us) per (candidate, env, step), K = %d, gamma = %.2f: median (min - max) of %d alternating blocks of >= 1 s of "
          "device time; rate in candidate-env-steps / s from the median\n" % (K, GAMMA, ROUNDS))
    print("| agents x envs x candidates | fused | fused again | baseline | replay | fused rate | baseline rate | baseline / fused | "
          "bytes per step fused / baseline | max rel. difference of the returns |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for i, (N, B, C) in enumerate(SHAPES):
        t, err = shape(N, B, C, with_replay=(i == 0))
        cell = lambda v: "%.4g (%.4g - %.4g)" % v
        fb, bb = bytes_per_step(N, C)
        print("| %d x %d x %d | %s | %s | %s | %s | %.3g | %.3g | %.2f | %.0f / %.0f | %.1e |"
              % (N, B, C, cell(t["fused"]), cell(t["fused_again"]), cell(t["baseline"]),
                 cell(t["replay"]) if "replay" in t else "-", 1e9 / t["fused"][0], 1e9 / t["baseline"][0],
                 t["baseline"][0] / t["fused"][0], fb, bb, err), flush=True)


if __name__ == "__main__":
    main()
