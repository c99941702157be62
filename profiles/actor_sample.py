#!/usr/bin/env python3
"""The exploring actor loop `a = mean(o) + exp(log_std) eps; o, r, d, info = env.step(a)`, us per env step (K = 20 steps per
call):

  sample     env.rollout_actor(K, GaussianActor(mean, log_std)): ONE actor_sample_kernel launch (fg_rollout_hd_actor_sample)
  fused      env.rollout_actor(K, mean): the deterministic actor_rollout_kernel, for the cost of sampling
  captured   FormationVecEnv.capture(policy, K) with policy(o) = mean(o) + exp(log_std) * torch.randn_like(mean(o)), the
             torch loop captured once in a hipGraph and replayed

mean = Sequential(Linear(6N, H), ReLU, Linear(H, H), ReLU, Linear(H, 2), Tanh), log_std = -0.5.  Every measurement runs in
a process of its own (`--one MODE N B H`): ~1 s of the same work to warm the clocks, then the median of 7 timed blocks.
Usage:  python3 profiles/actor_sample.py            (the table, markdown on stdout)
Kernel time: rocprofv3 --kernel-trace --stats -- python3 profiles/actor_sample.py --one sample 9 4096 64  (and fused)."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-formation_amd")]

K = 20
SHAPES = ((9, 4096), (27, 4096))
HIDDEN = (64,)
MODES = ("sample", "fused", "captured")


def one(mode, N, B, H):
    import torch
    import formation_gym
    from formation_gym.vec_env import FormationVecEnv
    dev = "cuda:0"
    torch.manual_seed(0)
    mean = torch.nn.Sequential(torch.nn.Linear(6 * N, H), torch.nn.ReLU(), torch.nn.Linear(H, H), torch.nn.ReLU(),
                               torch.nn.Linear(H, 2), torch.nn.Tanh()).to(dev)
    actor = formation_gym.GaussianActor(mean, torch.nn.Parameter(torch.full((2,), -0.5, device=dev)))
    env = formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device=dev)
    env.seed(1)
    venv = FormationVecEnv(env, reset_mode="device")
    venv.reset()
    env.world.step_count.copy_((torch.arange(B, device=dev) % 100).int())     # episodes end at different steps
    if mode == "sample":
        assert env.actor_path(actor) == "fused"
        body = lambda: env.rollout_actor(K, actor)                               # noqa: E731
    elif mode == "fused":
        assert env.actor_path(mean) == "fused"
        body = lambda: env.rollout_actor(K, mean)                                # noqa: E731
    else:
        def policy(o):
            mu = mean(o)
            return mu + torch.exp(actor.log_std) * torch.randn_like(mu)
        loop = venv.capture(policy, K)
        body = loop.replay
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
    print("| shape | H | sampling us/step | deterministic us/step | captured sampling loop us/step | sampling / deterministic | "
          "sampling / captured |")
    print("|---|---|---|---|---|---|---|")
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
            print("| %d x %d | %d | %.2f | %.2f | %.2f | %.3f | %.2f |" % (
                N, B, H, t["sample"], t["fused"], t["captured"], t["sample"] / t["fused"], t["sample"] / t["captured"]),
                flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 6 and sys.argv[1] == "--one":
        print("%.4f" % one(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])))
    else:
        main()
