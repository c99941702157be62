#!/usr/bin/env python3
"""The exploring loop of the MADDPG trainers' discrete-action policy (Gumbel-softmax, hard), us per env step (K = 20 steps per
call), for the four fused families - plain, bn (behind an eval-mode input BatchNorm), pa (one network per agent), pa_bn:

  <fam>_gumbel    env.rollout_actor(K, GumbelSoftmaxActor(logits)) on an env with discrete_action_space (FG_ACT_ONEHOT5), exploring:
                  ONE gumbel_actor_kernel / bn_gumbel_actor_kernel / pa_gumbel_actor_kernel / pa_bn_gumbel_actor_kernel launch
                  (fg_rollout_hd_actor_gumbel[_per_agent])
  <fam>_det       env.rollout_actor(K, actor) of the same body with a two-output head on a continuous env: the same family's
                  deterministic member (actor_rollout_kernel / bn_actor_kernel / pa_actor_kernel / pa_bn_actor_kernel) - what the
                  five-output head, the two Philox blocks, the ten logarithms and the pick cost on top of it
  <fam>_captured  FormationVecEnv.capture(policy, K), policy(o) = decode(one_hot(argmax(logits(o) - log(-log(rand))))): the torch
                  loop of the same policy - logits, argmax(logits + g), one-hot, the env's (a1 - a2, a3 - a4), env.step - captured
                  once in a hipGraph and replayed

logits = Sequential([BatchNorm,] Linear(6N, H), ReLU, Linear(H, H), ReLU, Linear(H, 5)) in eval mode with non-trivial running
statistics.  One process per shape (`--one N B H`): every variant is built and warmed (~1 s each), then the variants ALTERNATE
for ROUNDS rounds, one timed block (ending in a device synchronise) per variant and round; each variant is reported as the
median of its blocks with their min - max, the run-to-run spread inside the process.
Usage:  python3 profiles/actor_gumbel.py            (the table, markdown on stdout)"""
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
FAMILIES = ("plain", "bn", "pa", "pa_bn")
KINDS = ("gumbel", "det", "captured")
MODES = tuple(f + "_" + k for f in FAMILIES for k in KINDS)
ROUNDS = 7


def one(N, B, H):
    import torch
    import formation_gym
    from formation_gym.vec_env import FormationVecEnv
    nn = torch.nn
    dev = "cuda:0"
    torch.manual_seed(0)
    D = 6 * N

    def member(norm, head):
        mods = [nn.Linear(D, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, head)]
        if norm is not None:
            bn = norm(D)
            with torch.no_grad():
                bn.running_mean.normal_(0.0, 0.5)
                bn.running_var.uniform_(0.25, 4.0)
                bn.weight.uniform_(0.5, 1.5)
                bn.bias.normal_(0.0, 0.5)
            mods = [bn] + mods
        return nn.Sequential(*mods).to(dev).eval()

    def net(fam, head):
        bn = fam in ("bn", "pa_bn")
        if fam in ("pa", "pa_bn"):
            return formation_gym.PerAgentActor([member(nn.BatchNorm1d if bn else None, head) for _ in range(N)]).eval()
        return member(formation_gym.InputBatchNorm if bn else None, head)

    def make(mode):
        fam, kind = mode.rsplit("_", 1)
        if kind != "gumbel":
            env = formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device=dev)
        else:                                                                     # discrete_action_space: FG_ACT_ONEHOT5
            sc = formation_gym.load_scenario("formation_hd_env")
            world = sc.make_world(N, num_envs=B, device=dev)
            env = formation_gym.MultiAgentEnv(world, sc.reset_world, sc.reward, sc.observation, discrete_action=True)
        env.seed(1)
        venv = FormationVecEnv(env, reset_mode="device")
        venv.reset()
        env.world.step_count.copy_((torch.arange(B, device=dev) % 100).int())     # episodes end at different steps
        if kind == "captured":
            logits = net(fam, 5)

            def policy(o):
                lg = logits(o)
                u = torch.rand_like(lg).clamp_(1e-7, 1.0 - 1e-7)
                oh = torch.nn.functional.one_hot((lg - torch.log(-torch.log(u))).argmax(-1), 5).to(lg.dtype)
                return torch.stack((oh[..., 1] - oh[..., 2], oh[..., 3] - oh[..., 4]), -1)
            return venv.capture(policy, K).replay
        if kind == "gumbel":
            actor = formation_gym.GumbelSoftmaxActor(net(fam, 5), explore=True)
        else:
            actor = net(fam, 2)
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
            print("\n%d x %d, H = %d, us per env step: median (min - max) of %d alternating blocks\n" % (N, B, H, ROUNDS))
            print("| family | Gumbel | deterministic | captured torch loop | Gumbel / deterministic | Gumbel / captured |")
            print("|---|---|---|---|---|---|")
            for fam in FAMILIES:
                g, d, c = (t[fam + "_" + k] for k in KINDS)
                print("| %s | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) | %.2f (%.2f - %.2f) | %.3f | %.2f |"
                      % ((fam,) + g + d + c + (g[0] / d[0], g[0] / c[0])), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--one":
        for mode, v in one(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])).items():
            print("%s %.4f %.4f %.4f" % ((mode,) + v))
    else:
        main()
