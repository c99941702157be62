#!/usr/bin/env python3
"""The learned-actor loop `a = actor(o); o, r, d, info = env.step(a)` in the landmark scenarios four ways, us per env step
(K = 20 steps per call):

  fused      env.rollout_actor(K, actor): ONE launch, the actor inside the one-env-per-lane kernel (fg_rollout_scenario_actor)
  captured   FormationVecEnv.capture(actor, K): the torch actor + step loop captured once in a hipGraph, replayed
  launches   the same loop launch by launch from Python
  floor      env.rollout(pre-staged actions): the open-loop rollout, the store-bound floor

actor = Sequential(Linear(D, H), ReLU, Linear(H, H), ReLU, Linear(H, 2), Tanh), D the scenario's observation width.  Every
measurement runs in a process of its own (`--one MODE SCENARIO N B H`); each warms the clocks for ~1 s of the same work, then
times 7 blocks and reports their median, minimum and maximum.  "fused faster than captured" means the fused cell's SLOWEST
block is below the captured cell's FASTEST one.
Usage:  python3 profiles/actor_landmark.py [--large | --small]     (the table, markdown on stdout; --large: the 65536-env
rows only, --small: the 4096-env rows only)"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-formation_amd")]

K = 20
SHAPES = (("basic_formation_env", 3), ("formation_hd_partial_env", 5), ("formation_hd_partial_range_env", 4),
          ("formation_hd_obs_env", 4))
BATCHES = (65536, 4096)
HIDDEN = (64, 32)
MODES = ("fused", "captured", "launches", "floor")


def one(mode, name, N, B, H):
    import torch
    import formation_gym
    from formation_gym.vec_env import FormationVecEnv
    dev = "cuda:0"
    torch.manual_seed(0)
    env = formation_gym.make_env(name, False, N, num_envs=B, device=dev)
    env.seed(1)
    D = env._out["obs"].shape[-1]
    actor = torch.nn.Sequential(torch.nn.Linear(D, H), torch.nn.ReLU(), torch.nn.Linear(H, H), torch.nn.ReLU(),
                                torch.nn.Linear(H, 2), torch.nn.Tanh()).to(dev)
    venv = FormationVecEnv(env, reset_mode="device")
    venv.reset()
    wl = int(env.world.world_length)
    env.world.step_count.copy_((torch.arange(B, device=dev) % wl).int())        # episodes end at different steps
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
    return statistics.median(blocks), min(blocks), max(blocks)


def main(batches):
    print("| scenario | shape | H | fused us/step (min-max) | captured us/step (min-max) | launch by launch us/step | "
          "open-loop floor us/step | fused / captured | fused max < captured min |")
    print("|---|---|---|---|---|---|---|---|---|")
    for B in batches:
        for name, N in SHAPES:
            for H in HIDDEN:
                t = {}
                for mode in MODES:
                    r = subprocess.run([sys.executable, __file__, "--one", mode, name, str(N), str(B), str(H)],
                                       capture_output=True, text=True, timeout=300)
                    if r.returncode != 0:
                        sys.stderr.write(r.stderr[-2000:])
                        raise SystemExit("%s %s %d x %d H %d failed (%d)" % (mode, name, N, B, H, r.returncode))
                    t[mode] = [float(x) for x in r.stdout.strip().split()[-3:]]
                f, c = t["fused"], t["captured"]
                print("| %s | %d x %d | %d | %.2f (%.2f-%.2f) | %.2f (%.2f-%.2f) | %.2f | %.2f | %.2f | %s |" % (
                    name, N, B, H, f[0], f[1], f[2], c[0], c[1], c[2], t["launches"][0], t["floor"][0], f[0] / c[0],
                    "yes" if f[2] < c[1] else "no"), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 7 and sys.argv[1] == "--one":
        print("%.4f %.4f %.4f" % one(sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])))
    else:
        main(BATCHES[1:] if "--small" in sys.argv[1:] else BATCHES[:1] if "--large" in sys.argv[1:] else BATCHES)
