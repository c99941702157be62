"""16-bit observations out of the rollout launch: the figures of profiles/obs16.md.

One process; per shape the four variants
    a  the fp32 launch                                   env.rollout(acts, out)
    b  the fp32 launch, then obs.to(dtype)               the 'cast' route, and what a caller does today
    c  the fused fp16 launch                             env.rollout(acts, out16, obs_dtype=torch.float16)
    d  the fused bf16 launch
are timed round by round in alternation (a b c d a b c d ...), every window from the same snapshot of the env with the same
actions, into the same ordinary (un-placed) caller-owned buffers, device events around `reps` launches.  Before that the
spread of the fp32 launch against itself is recorded: the same window `rounds` times in a row.
Bytes per env-step are the byte arithmetic of the launch (24 N^2 observation bytes in fp32, 12 N^2 in 16 bits, 53 N + 16 for
everything else; the cast pass reads 24 N^2 and writes 12 N^2 more), the fraction is of 8 TB/s.

    python profiles/obs16.py [--out FILE.json] [--rounds 7]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-formation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
import formation_gym  # noqa: E402

DEV = "cuda:0"
PEAK = 8.0e12
# (agents, envs, steps per launch, closed loop, launches per timed window)
SHAPES = [(27, 4096, 20, False, 60), (9, 4096, 128, False, 60), (3, 16384, 20, False, 200), (27, 4096, 20, True, 60)]


def bytes_per_env_step(N, variant):
    rest = 53 * N + 16
    return {"a": 24 * N * N + rest, "b": 24 * N * N + rest + 36 * N * N, "c": 12 * N * N + rest, "d": 12 * N * N + rest}[variant]


def buffers(B, N, K, dtype, policy):
    f = dict(dtype=torch.float32, device=DEV)
    out = dict(obs=torch.empty((K, B, N, 6 * N), dtype=dtype, device=DEV), reward=torch.empty((K, B, N), **f),
               indiv=torch.empty((K, B, N), **f), done=torch.zeros((K, B, N), dtype=torch.uint8, device=DEV))
    if policy:
        out["act"] = torch.empty((K, B, N, 2), **f)
    return out


def measure(N, B, K, policy, reps, rounds):
    env = formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device=DEV)
    env.seed(1)
    env.reset()
    env.auto_reset = True
    g = torch.Generator().manual_seed(0)
    acts = (torch.rand((K, B, N, 2), generator=g) * 2 - 1).to(DEV)
    out32 = buffers(B, N, K, torch.float32, policy)
    out16 = {torch.float16: buffers(B, N, K, torch.float16, policy), torch.bfloat16: buffers(B, N, K, torch.bfloat16, policy)}
    snap = env._snapshot()

    def launch(out, dtype=None):
        if policy:
            return env.rollout_policy(K, 3, out=out, obs_dtype=dtype)
        return env.rollout(acts, out=out, obs_dtype=dtype)

    variants = {
        "a": lambda: launch(out32),
        "b": lambda: launch(out32)[0].to(torch.float16),
        "c": lambda: launch(out16[torch.float16], torch.float16),
        "d": lambda: launch(out16[torch.bfloat16], torch.bfloat16),
    }
    for dtype in out16:
        assert env.obs_path(dtype, policy=policy) == "fused"

    def window(fn):
        env._restore(snap)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) * 1e3 / (reps * K)                  # us per step

    for fn in variants.values():                                         # warm-up: code objects, bindings, the allocator's blocks
        window(fn)
    spread = [window(variants["a"]) for _ in range(rounds)]
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(window(fn))
    # the results the timed launches left: the fused bits are the cast's bits at this size too
    env._restore(snap)
    ref = launch(out32)[0]
    same = {}
    for dtype, o in out16.items():
        env._restore(snap)
        got = launch(o, dtype)[0]
        same[str(dtype)] = bool(torch.equal(got.view(torch.int16), ref.to(dtype).view(torch.int16)))
    med = lambda xs: sorted(xs)[len(xs) // 2]
    rows = {}
    for k, xs in times.items():
        by = bytes_per_env_step(N, k)
        rows[k] = dict(us_per_step=med(xs), lo=min(xs), hi=max(xs), bytes_per_env_step=by,
                       fraction_of_8TBs=by * B / (med(xs) * 1e-6) / PEAK)
    return dict(N=N, B=B, K=K, closed_loop=policy, reps=reps, fp32_spread=dict(lo=min(spread), hi=max(spread), median=med(spread),
                                                                             rel=(max(spread) - min(spread)) / med(spread)),
                variants=rows, bits_equal_cast=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "profiles/obs16.py needs a GPU"
    results = []
    for N, B, K, policy, reps in SHAPES:
        r = measure(N, B, K, policy, reps, args.rounds)
        results.append(r)
        s = r["fp32_spread"]
        print("%d x %d x %d %s: fp32 spread %.3f-%.3f us/step (%.2f %%), bits equal the cast: %s"
              % (N, B, K, "closed loop" if policy else "open loop", s["lo"], s["hi"], 100 * s["rel"], r["bits_equal_cast"]))
        a = r["variants"]["a"]["us_per_step"]
        for k, v in r["variants"].items():
            print("   %s  %8.3f us/step (%.3f-%.3f)  %6d B/env-step  %.3f of 8 TB/s  %.3f of (a)  %.3f of (b)"
                  % (k, v["us_per_step"], v["lo"], v["hi"], v["bytes_per_env_step"], v["fraction_of_8TBs"], v["us_per_step"] / a,
                     v["us_per_step"] / r["variants"]["b"]["us_per_step"]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
