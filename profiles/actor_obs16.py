"""16-bit observations out of the fused actor launch: the figures of profiles/actor_obs16.md.

One process; per (shape, actor) the four variants
    a  the fp32 fused actor launch                       env.rollout_actor(K, actor, out)
    b  (a), then obs.to(torch.float16)                   the 'cast' route, and what a trainer does without obs_dtype
    c  the fused fp16 launch                             env.rollout_actor(K, actor, out16, obs_dtype=torch.float16)
    d  the fused bf16 launch
are timed round by round in alternation (a b c d a b c d ...), every window from the same snapshot of the env and the same
hidden state, into the same ordinary caller-owned buffers, device events around `reps` launches.  Before that the spread of the
fp32 launch against itself is recorded: the same window `rounds` times in a row.  After the timing the fused bits are compared
with the cast's at the timed size.  The actors are the MAPPO trainers' LayerNorm actor and rMAPPO's recurrent one, H = 64, under a
GaussianActor.

    python profiles/actor_obs16.py [--out FILE.json] [--rounds 7]"""
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
from formation_gym import GaussianActor, RecurrentActor  # noqa: E402

nn = torch.nn
DEV = "cuda:0"
H = 64
# (agents, envs, steps per launch, launches per timed window)
SHAPES = [(3, 16384, 20, 20), (9, 4096, 20, 20), (27, 4096, 20, 20)]
MEMBERS = ("layernorm", "recurrent")


def make_actor(member, N):
    torch.manual_seed(0)
    D = 6 * N
    base = [nn.LayerNorm(D), nn.Linear(D, H), nn.ReLU(), nn.LayerNorm(H), nn.Linear(H, H), nn.ReLU(), nn.LayerNorm(H)]
    if member == "layernorm":
        mean = nn.Sequential(*(base + [nn.Linear(H, 2)]))
    else:
        mean = RecurrentActor(nn.Sequential(*base), nn.GRUCell(H, H), nn.LayerNorm(H), nn.Linear(H, 2))
    return GaussianActor(mean, nn.Parameter(torch.tensor([-0.5, -0.5]))).to(DEV)


def buffers(B, N, K, dtype):
    f = dict(dtype=torch.float32, device=DEV)
    return dict(obs=torch.empty((K, B, N, 6 * N), dtype=dtype, device=DEV), reward=torch.empty((K, B, N), **f),
                indiv=torch.empty((K, B, N), **f), done=torch.zeros((K, B, N), dtype=torch.uint8, device=DEV),
                act=torch.empty((K, B, N, 2), **f), log_prob=torch.empty((K, B, N), **f))


def measure(member, N, B, K, reps, rounds):
    env = formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device=DEV)
    env.seed(1)
    env.reset()
    env.auto_reset = True
    actor = make_actor(member, N)
    assert env.actor_path(actor) == "fused"
    recurrent = member == "recurrent"
    h0 = (torch.rand((B, N, H), generator=torch.Generator().manual_seed(0)) - 0.5).to(DEV) if recurrent else None
    h = h0.clone() if recurrent else None
    out32 = buffers(B, N, K, torch.float32)
    out16 = {torch.float16: buffers(B, N, K, torch.float16), torch.bfloat16: buffers(B, N, K, torch.bfloat16)}
    snap = env._snapshot()
    for dtype in out16:
        assert env.obs_path(dtype, actor=actor) == "fused", (member, N, dtype)

    def launch(out, dtype=None):
        return env.rollout_actor(K, actor, out=out, rnn_state=h, obs_dtype=dtype)

    variants = {
        "a": lambda: launch(out32),
        "b": lambda: launch(out32)[0].to(torch.float16),
        "c": lambda: launch(out16[torch.float16], torch.float16),
        "d": lambda: launch(out16[torch.bfloat16], torch.bfloat16),
    }

    def restore():
        env._restore(snap)
        if recurrent:
            h.copy_(h0)

    def window(fn):
        restore()
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
    # the results at the timed size: the fused bits are the cast's bits, everything else the fp32 launch's
    restore()
    ref = launch(out32)
    ref_obs, ref_logp, ref_act = ref[0].clone(), ref[3]["log_prob"].clone(), ref[3]["actions"].clone()
    same = {}
    for dtype, o in out16.items():
        restore()
        got = launch(o, dtype)
        same[str(dtype)] = bool(torch.equal(got[0].view(torch.int16), ref_obs.to(dtype).view(torch.int16))
                                and torch.equal(got[3]["log_prob"], ref_logp) and torch.equal(got[3]["actions"], ref_act))
    med = lambda xs: sorted(xs)[len(xs) // 2]
    rows = {k: dict(us_per_step=med(xs), lo=min(xs), hi=max(xs)) for k, xs in times.items()}
    return dict(member=member, N=N, B=B, K=K, H=H, reps=reps,
                fp32_spread=dict(lo=min(spread), hi=max(spread), median=med(spread), width=max(spread) - min(spread)),
                variants=rows, bits_equal_cast=same)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "profiles/actor_obs16.py needs a GPU"
    results = []
    for N, B, K, reps in SHAPES:
        for member in MEMBERS:
            r = measure(member, N, B, K, reps, args.rounds)
            results.append(r)
            s = r["fp32_spread"]
            print("%s %d x %d x %d: fp32 spread %.3f-%.3f us/step (width %.3f), bits equal the cast: %s"
                  % (member, N, B, K, s["lo"], s["hi"], s["width"], r["bits_equal_cast"]))
            v = r["variants"]
            for k, x in v.items():
                print("   %s  %8.3f us/step (%.3f-%.3f)  %.3f of (a)  %.3f of (b)  (b) - this = %.3f us"
                      % (k, x["us_per_step"], x["lo"], x["hi"], x["us_per_step"] / v["a"]["us_per_step"],
                         x["us_per_step"] / v["b"]["us_per_step"], v["b"]["us_per_step"] - x["us_per_step"]), flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
