#!/usr/bin/env python3
"""The learned-actor loop `a = actor(o); o, r, d, info = env.step(a)` four ways, us per env step (K = 20 steps per call):

  fused      env.rollout_actor(K, actor): ONE launch, the actor inside the rollout kernel (fg_rollout_hd_actor)
  captured   FormationVecEnv.capture(actor, K): the torch actor + step loop captured once in a hipGraph, replayed
  launches   the same loop launch by launch from Python
  floor      env.rollout(pre-staged actions): the open-loop rollout, the store-bound floor

actor = Sequential(Linear(6N, H), ReLU, Linear(H, H), ReLU, Linear(H, 2), Tanh), one per run.  Every measurement runs in a
process of its own (`--one MODE N B H`); each warms the clocks for ~1 s of the same work, then reports the median of 7 timed
blocks.  Usage:  python3 profiles/actor_rollout.py            (the whole table, markdown on stdout)"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-formation_amd")]

K = 20
SHAPES = ((9, 4096), (27, 4096), (8, 16384), (27, 256))
HIDDEN = (64, 128)
MODES = ("fused", "captured", "launches", "floor")


def one(mode, N, B, H):
    import torch
    import formation_gym
    from formation_gym.vec_env import FormationVecEnv
    dev = "cuda:0"
    torch.manual_seed(0)
    actor = torch.nn.Sequential(torch.nn.Linear(6 * N, H), torch.nn.ReLU(), torch.nn.Linear(H, H), torch.nn.ReLU(),
                                torch.nn.Linear(H, 2), torch.nn.Tanh()).to(dev)
    env = formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device=dev)
    env.seed(1)
    venv = FormationVecEnv(env, reset_mode="device")
    venv.reset()
    env.world.step_count.copy_((torch.arange(B, device=dev) % 100).int())     # episodes end at different steps
    if mode == "fused":
        assert env.actor_path(actor) == "fused"
        body = lambda: env.rollout_actor(K, actor)                               # noqa: E731
    elif mode == "captured":
        loop = venv.capture(actor, K)
        body = loop.replay
    elif mode == "launches":
        state = {"obs": env._out["obs"]}

        def body():
            with torch.no_grad():
                for _ in range(K):
                    state["obs"] = venv.step(actor(state["obs"]))[0]
    else:
        acts = torch.rand((K, B, N, 2), device=dev) * 2 - 1
        body = lambda: env.rollout(acts)                                         # noqa: E731
    body()
    torch.cuda.synchronize()
    t_end = time.perf_counter() + 1.0                                            # warm clocks
    n_warm = 0
    while time.perf_counter() < t_end:
        body(); n_warm += 1
        if n_warm % 8 == 0:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    reps = max(5, min(200, n_warm // 4))
    blocks = []
    for _ in range(7):
        t0 = time.perf_counter()
        for _ in range(reps):
            body()
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t0) / (reps * K) * 1e6)
    return statistics.median(blocks)


def main():
    print("| shape | H | fused us/step | captured us/step | launch by launch us/step | open-loop floor us/step | "
          "fused / captured | actor TFLOP/s (of 157) | obs GB/s (of 8000) |")
    print("|---|---|---|---|---|---|---|---|---|")
    for N, B in SHAPES:
        for H in HIDDEN:
            t = {}
            for mode in MODES:
                r = subprocess.run([sys.executable, __file__, "--one", mode, str(N), str(B), str(H)], capture_output=True,
                                   text=True, timeout=600)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr[-2000:])
                    raise SystemExit("%s %d x %d H %d failed (%d)" % (mode, N, B, H, r.returncode))
                t[mode] = float(r.stdout.strip().split()[-1])
            flop = 2.0 * (6 * N * H + H * H + 2 * H) * B * N                       # per step, the whole 6N-column input
            obs_bytes = 24.0 * N * N * B
            print("| %d x %d | %d | %.2f | %.2f | %.2f | %.2f | %.2f | %.1f | %.0f |" % (
                N, B, H, t["fused"], t["captured"], t["launches"], t["floor"], t["fused"] / t["captured"],
                flop / t["fused"] * 1e-6, obs_bytes / t["fused"] * 1e-3), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 6 and sys.argv[1] == "--one":
        print("%.4f" % one(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])))
    else:
        main()
