#!/usr/bin/env python3
"""One CEM control step (ITERATIONS rounds of: draw C candidates around (mean, std), score them from the current state, refit mean
and std to each row's E best): `formation_gym.CEMPlanner` against what a user of `env.rollout_returns` writes in torch.

  torch        per iteration torch.randn, mean + std * eps, clamp, env.rollout_returns, topk over C, gather, mean, std; the
               shift of the plan at the end: the [C, K, B, N, 2] tensor is written in several passes and read three more times
  torch_again  the same leg a second time in the alternation: the difference of the two medians is the run-to-run spread
  materialised fg_plan_candidates_std, env.rollout_returns, fg_plan_cem_update (CEMPlanner's route where no fused launch exists)
  fused        fg_rollout_hd_returns_sampled_std, fg_plan_cem_update: no candidate tensor
  mppi         MPPIPlanner.plan() at the same C: ONE scoring-plus-update pair (a CEM step is ITERATIONS such pairs)
  update_cem / update_mppi     the two update kernels alone on the same returns
  score_std / score_sampled    the two drawing scoring launches alone: returns_sampled_std_kernel against returns_sampled_kernel

One process: every leg of a shape is built and warmed, then the legs ALTERNATE for ROUNDS rounds; a round's block is a run of
calls, each between two device events, whose event times are summed; a leg is reported as the median of its blocks with their
min - max.  Peak extra device memory: torch.cuda.max_memory_allocated over one call, minus what was allocated before it.
Usage:  python3 profiles/planner_cem.py            (markdown on stdout)"""
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-formation_amd")]

K, ITERATIONS = 20, 3
GAMMA, SIGMA, LAM, CLIP = 0.97, 0.5, 1.0, 1.0
SHAPES = ((27, 4096, 8, 2), (9, 4096, 16, 4), (3, 16384, 16, 4), (27, 1, 4096, 400))      # (agents, envs, candidates, elites)
ROUNDS = 5
BLOCK_MS = 300.0


def shape(N, B, C, E):
    import torch
    import formation_gym
    from formation_gym import _native
    dev = "cuda:0"
    env = formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device=dev)
    env.seed(1)
    env.reset()
    assert env.returns_path() == "fused"
    fused = formation_gym.CEMPlanner(env, K, C, E, SIGMA, iterations=ITERATIONS, gamma=GAMMA, clip=CLIP)
    mat = formation_gym.CEMPlanner(env, K, C, E, SIGMA, iterations=ITERATIONS, gamma=GAMMA, clip=CLIP)
    mat.path = lambda: "materialised"
    mppi = formation_gym.MPPIPlanner(env, K, C, SIGMA, LAM, gamma=GAMMA, clip=CLIP)
    mean = [torch.zeros((K, B, N, 2), device=dev)]

    def torch_leg():
        m, s = mean[0], torch.full((K, B, N, 2), SIGMA, device=dev)
        for _ in range(ITERATIONS):
            u = torch.clamp(m[None] + s[None] * torch.randn((C, K, B, N, 2), device=dev), -CLIP, CLIP)
            ret, _ = env.rollout_returns(u, GAMMA)
            idx = torch.topk(ret, E, 0).indices                                          # [E, B, N]
            el = torch.gather(u, 0, idx[:, None, :, :, None].expand(E, K, B, N, 2))
            m, s = el.mean(0), el.std(0, unbiased=False)
        mean[0] = torch.cat([m[1:], m[-1:]], 0)
        return m[0]

    # the same results first: both routes, one control step
    a0, i0 = fused.plan()
    a1, i1 = mat.plan()
    assert torch.equal(a0, a1) and torch.equal(i0["std"], i1["std"]) and torch.equal(i0["elites"], i1["elites"])

    lib, st = _native.load(), _native.current_stream(torch.device(dev))
    out = dict(ret=torch.empty((C, B, N), device=dev), indiv=torch.empty((C, B, N), device=dev),
               steps=torch.empty((B,), dtype=torch.int32, device=dev))
    m_in = (torch.rand((K, B, N, 2), device=dev) - 0.5)
    s_in = torch.full((K, B, N, 2), SIGMA, device=dev)
    score_std = env.scenario.bind_rollout_returns_sampled_std(env.world, m_in, s_in, C, out)
    score_sampled = env.scenario.bind_rollout_returns_sampled(env.world, m_in, C, out, GAMMA)
    score_std(7, GAMMA, CLIP)
    ret = out["ret"].clone()
    score_sampled(7, SIGMA, CLIP)
    assert torch.equal(ret, out["ret"])                      # a constant std: the scalar launch's bits
    m_out, s_out, act = torch.empty_like(m_in), torch.empty_like(m_in), torch.empty((B, N, 2), device=dev)
    idx = torch.empty((E, B, N), dtype=torch.int32, device=dev)
    p = fused._params()

    def update_cem():
        _native.check(lib.fg_plan_cem_update(p, B, N, K, C, E, 7, CLIP, 1.0, 0.0, ret.data_ptr(), m_in.data_ptr(), s_in.data_ptr(),
                                             m_out.data_ptr(), s_out.data_ptr(), act.data_ptr(), idx.data_ptr(), 1, st))

    def update_mppi():
        _native.check(lib.fg_plan_mppi_update(p, B, N, K, C, 7, SIGMA, CLIP, LAM, ret.data_ptr(), m_in.data_ptr(),
                                              m_out.data_ptr(), act.data_ptr(), 1, st))

    legs = {"torch": torch_leg, "materialised": mat.plan, "fused": fused.plan, "torch_again": torch_leg, "mppi": mppi.plan,
            "update_cem": update_cem, "update_mppi": update_mppi,
            "score_std": lambda: score_std(7, GAMMA, CLIP), "score_sampled": lambda: score_sampled(7, SIGMA, CLIP)}

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
    print("us of device time per control step (mppi: per scoring-plus-update pair; update_* and score_*: per launch), K = %d, "
          "iterations = %d, sigma = %g: median (min - max) of %d alternating blocks of >= %.1f s of device time; peak extra device "
          "memory of one call in MiB\n" % (K, ITERATIONS, SIGMA, ROUNDS, BLOCK_MS / 1e3))
    print("| agents x envs x candidates, elites | torch | torch again | materialised | fused | torch / fused | mppi pair | "
          "fused / iterations | update_cem | update_mppi | score_std | score_sampled | std / sampled | "
          "peak MiB torch / materialised / fused |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for N, B, C, E in SHAPES:
        t, peak = shape(N, B, C, E)
        cell = lambda v: "%.4g (%.4g - %.4g)" % v
        print("| %d x %d x %d, %d | %s | %s | %s | %s | %.2f | %s | %.4g | %s | %s | %s | %s | %.3f | %.1f / %.1f / %.1f |"
              % (N, B, C, E, cell(t["torch"]), cell(t["torch_again"]), cell(t["materialised"]), cell(t["fused"]),
                 t["torch"][0] / t["fused"][0], cell(t["mppi"]), t["fused"][0] / ITERATIONS, cell(t["update_cem"]),
                 cell(t["update_mppi"]), cell(t["score_std"]), cell(t["score_sampled"]),
                 t["score_std"][0] / t["score_sampled"][0], peak["torch"], peak["materialised"], peak["fused"]), flush=True)


if __name__ == "__main__":
    main()
