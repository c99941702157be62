#!/usr/bin/env python3
"""One MPPI control step (draw C candidates around a plan, score them from the current state, average them by their returns):
`formation_gym.MPPIPlanner` against what a user of `env.rollout_returns` writes in torch.

  torch        torch.randn, mean + sigma * eps, clamp, env.rollout_returns, softmax((R - max) / lam) over C, the weighted sum
               over C, the shift of the plan: the [C, K, B, N, 2] tensor is written in several passes and read twice
  torch_again  the same leg a second time in the alternation: the difference of the two medians is the run-to-run spread
  materialised fg_plan_candidates, env.rollout_returns, fg_plan_mppi_update (MPPIPlanner's route where no fused launch exists)
  fused        fg_rollout_hd_returns_sampled, fg_plan_mppi_update: no candidate tensor
  score_sampled / score_read   the two scoring launches alone: returns_sampled_kernel (bound, drawing) against
               env.rollout_returns on the materialised tensor (returns_kernel)

One process: every leg of a shape is built and warmed, then the legs ALTERNATE for ROUNDS rounds; a round's block is a run of
calls, each between two device events, whose event times are summed; a leg is reported as the median of its blocks with their
min - max.  Peak extra device memory: torch.cuda.max_memory_allocated over one call, minus what was allocated before it.
Usage:  python3 profiles/planner_mppi.py            (markdown on stdout)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-formation_amd")]

K = 20
GAMMA, SIGMA, LAM, CLIP = 0.97, 0.5, 1.0, 1.0
SHAPES = ((27, 4096, 8), (9, 4096, 16), (3, 16384, 16), (27, 1, 4096))      # (agents, envs, candidates)
ROUNDS = 5
BLOCK_MS = 400.0


def shape(N, B, C):
    import torch
    import formation_gym
    dev = "cuda:0"
    env = formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device=dev)
    env.seed(1)
    env.reset()
    assert env.returns_path() == "fused"
    fused = formation_gym.MPPIPlanner(env, K, C, SIGMA, LAM, gamma=GAMMA, clip=CLIP)
    mat = formation_gym.MPPIPlanner(env, K, C, SIGMA, LAM, gamma=GAMMA, clip=CLIP)
    mat.path = lambda: "materialised"
    mean = [torch.zeros((K, B, N, 2), device=dev)]

    def torch_leg():
        eps = torch.randn((C, K, B, N, 2), device=dev)
        u = torch.clamp(mean[0][None] + SIGMA * eps, -CLIP, CLIP)
        ret, _ = env.rollout_returns(u, GAMMA)
        w = torch.softmax((ret - ret.max(0, keepdim=True).values) / LAM, 0)           # [C, B, N]
        new = (w[:, None, :, :, None] * u).sum(0)
        mean[0] = torch.cat([new[1:], new[-1:]], 0)
        return new[0]

    cands = fused.candidates()
    out = dict(ret=torch.empty((C, B, N), device=dev), indiv=torch.empty((C, B, N), device=dev),
               steps=torch.empty((B,), dtype=torch.int32, device=dev))
    bound = env.scenario.bind_rollout_returns_sampled(env.world, fused.mean, C, out, GAMMA)
    # the same results first: the sampled launch against the read one on the same candidates
    bound(fused.noise_offset, SIGMA, CLIP)
    assert torch.equal(out["ret"], env.rollout_returns(cands, GAMMA)[0])

    legs = {"torch": torch_leg, "materialised": mat.plan, "fused": fused.plan, "torch_again": torch_leg,
            "score_sampled": lambda: bound(7, SIGMA, CLIP), "score_read": lambda: env.rollout_returns(cands, GAMMA)}

    def timed(call, reps):
        pairs = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            pairs.append((e0, e1))
        torch.cuda.synchronize()
        return sum(x.elapsed_time(y) for x, y in pairs)      # ms of device time between the events

    reps, peak = {}, {}
    for name, call in legs.items():
        timed(call, 3)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        call()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20
        ms, n = 0.0, 0
        while ms < BLOCK_MS:
            ms += timed(call, 4); n += 4
        reps[name] = max(4, int(n * BLOCK_MS / ms) + 1)
    blocks = {name: [] for name in legs}
    for _ in range(ROUNDS):
        for name, call in legs.items():                      # the legs alternate
            blocks[name].append(timed(call, reps[name]) / reps[name] * 1e3)      # us per call
    return {name: (statistics.median(v), min(v), max(v)) for name, v in blocks.items()}, peak


def main():
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    print("us of device time per control step (score_*: per scoring launch), K = %d, sigma = %g, lam = %g: median (min - max) of %d "
          "alternating blocks of >= %.1f s of device time; peak extra device memory of one call in MiB\n"
          % (K, SIGMA, LAM, ROUNDS, BLOCK_MS / 1e3))
    print("| agents x envs x candidates | torch | torch again | materialised | fused | torch / fused | score_sampled | score_read | "
          "sampled / read | ns per candidate-env-step sampled / read | peak MiB torch / materialised / fused |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for N, B, C in SHAPES:
        t, peak = shape(N, B, C)
        cell = lambda v: "%.4g (%.4g - %.4g)" % v
        per = 1e3 / (C * B * K)
        print("| %d x %d x %d | %s | %s | %s | %s | %.2f | %s | %s | %.3f | %.4g / %.4g | %.1f / %.1f / %.1f |"
              % (N, B, C, cell(t["torch"]), cell(t["torch_again"]), cell(t["materialised"]), cell(t["fused"]),
                 t["torch"][0] / t["fused"][0], cell(t["score_sampled"]), cell(t["score_read"]),
                 t["score_sampled"][0] / t["score_read"][0], t["score_sampled"][0] * per, t["score_read"][0] * per,
                 peak["torch"], peak["materialised"], peak["fused"]), flush=True)


if __name__ == "__main__":
    main()
