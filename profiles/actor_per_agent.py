#!/usr/bin/env python3
"""Per-agent actors (one MLP per agent, MADDPG-style): the loop `a_i = actor_i(o_i); o, r, d, info = env.step(a)`, us per env
step (K = 20 steps per call):

  per_agent  env.rollout_actor(K, PerAgentActor([...])): ONE pa_actor_kernel launch (fg_rollout_hd_actor_per_agent)
  captured   FormationVecEnv.capture(policy, K), policy evaluating the N actors batched over agents: the weights stacked
             once outside the loop ([N, H, 6N] ...), each layer one torch.baddbmm over agents, the torch loop captured once
             in a hipGraph and replayed
  shared     env.rollout_actor(K, actor): the fused shared actor (actor_rollout_kernel) at the same shape

actor_i = Sequential(Linear(6N, H), ReLU, Linear(H, H), ReLU, Linear(H, 2), Tanh), PyTorch's default initialisation, a
different seed per agent.  Every measurement runs in a process of its own (`--one MODE N B H`): ~1 s of the same work to warm
the clocks, then the median of 7 timed blocks.
Usage:  python3 profiles/actor_per_agent.py            (the table, markdown on stdout)
Kernel time: rocprofv3 --kernel-trace --stats -- python3 profiles/actor_per_agent.py --one per_agent 9 4096 64  (and shared)."""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-formation_amd")]

K = 20
SHAPES = ((9, 4096), (27, 4096))
HIDDEN = (64, 128)
MODES = ("per_agent", "captured", "shared")


def _mlp(N, H, seed, dev):
    import torch
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(6 * N, H), torch.nn.ReLU(), torch.nn.Linear(H, H), torch.nn.ReLU(),
                               torch.nn.Linear(H, 2), torch.nn.Tanh()).to(dev)


def one(mode, N, B, H):
    import torch
    import formation_gym
    from formation_gym.vec_env import FormationVecEnv
    dev = "cuda:0"
    pa = formation_gym.PerAgentActor([_mlp(N, H, 1000 + i, dev) for i in range(N)])
    env = formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device=dev)
    env.seed(1)
    venv = FormationVecEnv(env, reset_mode="device")
    venv.reset()
    env.world.step_count.copy_((torch.arange(B, device=dev) % 100).int())     # episodes end at different steps
    if mode == "per_agent":
        assert env.actor_path(pa) == "fused"
        body = lambda: env.rollout_actor(K, pa)                                  # noqa: E731
    elif mode == "shared":
        shared = pa.actors[0]
        assert env.actor_path(shared) == "fused"
        body = lambda: env.rollout_actor(K, shared)                              # noqa: E731
    else:
        # stacked once: W [N, out, in] -> [N, in, out] for baddbmm over agents, biases [N, 1, out]
        def stack(j):
            w = torch.stack([a[j].weight.detach() for a in pa.actors]).transpose(1, 2).contiguous()
            b = torch.stack([a[j].bias.detach() for a in pa.actors]).unsqueeze(1).contiguous()
            return w, b
        (w1, b1), (w2, b2), (w3, b3) = stack(0), stack(2), stack(4)

        def policy(o):                                                           # o [B, N, 6N]
            x = o.transpose(0, 1)                                                # [N, B, 6N]
            h = torch.relu(torch.baddbmm(b1, x, w1))
            h = torch.relu(torch.baddbmm(b2, h, w2))
            return torch.tanh(torch.baddbmm(b3, h, w3)).transpose(0, 1)          # [B, N, 2]
        with torch.no_grad():
            o = torch.randn(5, N, 6 * N, device=dev)
            assert torch.allclose(policy(o), pa(o), atol=1e-5)
        loop = venv.capture(policy, K)
        body = loop.replay
    with torch.no_grad():
        body()
        torch.cuda.synchronize()
        t_end = time.perf_counter() + 1.0                                        # warm clocks
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
    print("| shape | H | per-agent fused us/step | captured per-agent loop us/step | shared fused us/step | "
          "per-agent / captured | per-agent / shared |")
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
            print("| %d x %d | %d | %.2f | %.2f | %.2f | %.2f | %.2f |" % (
                N, B, H, t["per_agent"], t["captured"], t["shared"], t["per_agent"] / t["captured"],
                t["per_agent"] / t["shared"]), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 6 and sys.argv[1] == "--one":
        print("%.4f" % one(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])))
    else:
        main()
