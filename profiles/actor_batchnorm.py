#!/usr/bin/env python3
"""The exploring loop of the MADDPG trainers' BatchNorm actor (eval mode), us per env step (K = 20 steps per call):

  bn            env.rollout_actor(K, GaussianActor(bn_mean, log_std)): ONE bn_sample_kernel launch (fg_rollout_hd_actor_bn)
  plain         the same Linears without the norm: actor_sample_kernel - the difference is the whole-k layer 1 plus the
                normalisation
  pa_bn         one BatchNorm actor per agent: ONE pa_bn_sample_kernel launch (fg_rollout_hd_actor_bn_per_agent)
  pa_plain      the members without their norms: pa_sample_kernel
  captured      FormationVecEnv.capture(policy, K), policy(o) = bn_mean(o) + exp(log_std) * randn: the torch loop over the
                shared BatchNorm actor captured once in a hipGraph and replayed
  pa_captured   the same over the PerAgentActor of BatchNorm members

bn_mean = Sequential(InputBatchNorm(6N), Linear(6N, H), ReLU, Linear(H, H), ReLU, Linear(H, 2)) in eval mode with non-trivial
running statistics, log_std = -0.5.  One process per shape (`--one N B H`): every variant is built and warmed (~1 s each), then
the variants ALTERNATE for ROUNDS rounds, one timed block (ending in a device synchronise) per variant and round; each variant
is reported as the median of its blocks with their min - max, the run-to-run spread inside the process.
Usage:  python3 profiles/actor_batchnorm.py            (the table, markdown on stdout)
Kernel time: rocprofv3 --kernel-trace --stats -- python3 profiles/actor_batchnorm.py --one 9 4096 64."""
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
MODES = ("bn", "plain", "pa_bn", "pa_plain", "captured", "pa_captured")
ROUNDS = 7


def one(N, B, H):
    import torch
    import formation_gym
    from formation_gym.vec_env import FormationVecEnv
    nn = torch.nn
    dev = "cuda:0"
    torch.manual_seed(0)
    D = 6 * N

    def member(norm):
        bn = norm(D)
        with torch.no_grad():
            bn.running_mean.normal_(0.0, 0.5)
            bn.running_var.uniform_(0.25, 4.0)
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.normal_(0.0, 0.5)
        lin = [nn.Linear(D, H), nn.Linear(H, H), nn.Linear(H, 2)]
        body = [lin[0], nn.ReLU(), lin[1], nn.ReLU(), lin[2]]
        return nn.Sequential(bn, *body).to(dev).eval(), nn.Sequential(*body).to(dev)

    bn_mean, mean = member(formation_gym.InputBatchNorm)
    members = [member(nn.BatchNorm1d) for _ in range(N)]
    pa_bn_mean = formation_gym.PerAgentActor([m[0] for m in members]).eval()
    pa_mean = formation_gym.PerAgentActor([m[1] for m in members])
    log_std = nn.Parameter(torch.full((2,), -0.5, device=dev))

    def make(mode):
        env = formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device=dev)
        env.seed(1)
        venv = FormationVecEnv(env, reset_mode="device")
        venv.reset()
        env.world.step_count.copy_((torch.arange(B, device=dev) % 100).int())     # episodes end at different steps
        if mode in ("captured", "pa_captured"):
            net = bn_mean if mode == "captured" else pa_bn_mean

            def policy(o):
                mu = net(o)
                return mu + torch.exp(log_std) * torch.randn_like(mu)
            return venv.capture(policy, K).replay
        actor = formation_gym.GaussianActor({"bn": bn_mean, "plain": mean, "pa_bn": pa_bn_mean, "pa_plain": pa_mean}[mode], log_std)
        assert env.actor_path(actor) == "fused", mode
        return lambda: env.rollout_actor(K, actor)

    bodies, reps = {}, {}
    for mode in MODES:
        body = bodies[mode] = make(mode)
        body()
        torch.cuda.synchronize()
        t_end, n_warm = time.perf_counter() + 1.0, 0                              # warm clocks
        while time.perf_counter() < t_end:
            body(); n_warm += 1
            if n_warm % 8 == 0:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        reps[mode] = max(5, min(200, n_warm // 4))
    blocks = {mode: [] for mode in MODES}
    for _ in range(ROUNDS):
        for mode in MODES:                                                       # the variants alternate
            body = bodies[mode]
            t0 = time.perf_counter()
            for _ in range(reps[mode]):
                body()
            torch.cuda.synchronize()
            blocks[mode].append((time.perf_counter() - t0) / (reps[mode] * K) * 1e6)
    return {mode: (statistics.median(v), min(v), max(v)) for mode, v in blocks.items()}


def main():
    print("| shape | H | " + " | ".join("%s us/step (min - max)" % m for m in MODES) + " | bn / plain | pa_bn / pa_plain | "
          "bn / captured | pa_bn / pa_captured |")
    print("|---|---|" + "---|" * (len(MODES) + 4))
    for N, B in SHAPES:
        for H in HIDDEN:
            r = subprocess.run([sys.executable, __file__, "--one", str(N), str(B), str(H)], capture_output=True, text=True,
                               timeout=900)
            if r.returncode != 0:
                sys.stderr.write(r.stderr[-2000:])
                raise SystemExit("%d x %d H %d failed (%d)" % (N, B, H, r.returncode))
            t = {}
            for line in r.stdout.splitlines():
                f = line.split()
                if len(f) == 4 and f[0] in MODES:
                    t[f[0]] = tuple(float(x) for x in f[1:])
            cells = " | ".join("%.2f (%.2f - %.2f)" % t[m] for m in MODES)
            print("| %d x %d | %d | %s | %.3f | %.3f | %.2f | %.2f |" % (
                N, B, H, cells, t["bn"][0] / t["plain"][0], t["pa_bn"][0] / t["pa_plain"][0], t["bn"][0] / t["captured"][0],
                t["pa_bn"][0] / t["pa_captured"][0]), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--one":
        for mode, v in one(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])).items():
            print("%s %.4f %.4f %.4f" % ((mode,) + v))
    else:
        main()
