#!/usr/bin/env python3
"""The sampling loop of the MAPPO / rMAPPO trainers' discrete-action policy, us per env step (K = 20 steps per call), for the
three fused families - plain, LayerNorm (ln), recurrent (gru):

  <fam>_cat       env.rollout_actor(K, CategoricalActor(logits)) on an env with discrete_action_input: ONE cat_actor_kernel /
                  ln_cat_actor_kernel / gru_cat_actor_kernel launch (fg_rollout_hd_actor_cat)
  <fam>_gauss     env.rollout_actor(K, GaussianActor(mean, log_std)) of the same body with a two-output head on a continuous
                  env: actor_sample_kernel / ln_sample_kernel / gru_sample_kernel, the same family's Gaussian member - the same
                  Philox block per (env, agent) and step; the difference is five fmaf chains per lane against one, the softmax
                  CDF pick against exp(log_std) eps, and two more [K, B, N] outputs
  <fam>_captured  FormationVecEnv.capture(policy, K), policy(o) = table[sample(softmax(logits(o)))]: the torch loop of the
                  same categorical policy - sample, decode to the raw action, env.step - captured once in a hipGraph and
                  replayed.  The sample is the inverse CDF, (rand >= cumsum(softmax)[..., :4]).sum(-1), the fused kernels'
                  rule in torch ops: Categorical(logits).sample() is torch.multinomial, which checks its input on the host
                  (a device synchronise) and so cannot be captured.  The recurrent policy keeps its state in a tensor and
                  does not see the done flags, so it never masks it: less work than the fused launch does

`--parent-lib PATH` also measures the *_gauss variants with the library at PATH (a build of the parent commit) in child
processes of their own, alternating with the children that load this tree's library: `parent_<fam>_gauss`.
One process per (shape, library) and outer round (`--one N B H [LIB]`): every variant is built and warmed (~1 s each), then
the variants ALTERNATE for ROUNDS rounds, one timed block (ending in a device synchronise) per variant and round; a variant is
reported as the median of its blocks over all outer rounds with their min - max, the run-to-run spread.
Usage:  python3 profiles/actor_categorical.py [--parent-lib PATH]            (the table, markdown on stdout)"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "gym-formation_amd")]

K = 20
SHAPES = ((9, 4096), (27, 4096))
H = 64
FAMILIES = ("plain", "ln", "gru")
ROUNDS = 7
OUTER = 2


def one(N, B, H, lib=None):
    import torch
    import formation_gym
    from formation_gym import _native
    from formation_gym.vec_env import FormationVecEnv
    if lib:                                        # a parent build: without the entries this tree adds
        _native.LIB_PATH = lib
        for name in ("fg_rollout_hd_actor_cat", "fg_describe_actor_cat_launch", "fg_actor_uniform", "fg_actor_categorical"):
            _native.SIGNATURES.pop(name, None)
    nn = torch.nn
    dev = "cuda:0"
    D = 6 * N
    parent = bool(lib)
    modes = [f + "_gauss" for f in FAMILIES] if parent else [f + m for f in FAMILIES for m in ("_cat", "_gauss", "_captured")]

    def body_mods(fam):
        if fam == "plain":
            return [nn.Linear(D, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU()]
        return [nn.LayerNorm(D), nn.Linear(D, H), nn.ReLU(), nn.LayerNorm(H), nn.Linear(H, H), nn.ReLU(), nn.LayerNorm(H)]

    def net(fam, head):
        torch.manual_seed(0)
        if fam == "gru":
            return formation_gym.RecurrentActor(nn.Sequential(*body_mods(fam)), nn.GRUCell(H, H), nn.LayerNorm(H),
                                                nn.Linear(H, head)).to(dev)
        return nn.Sequential(*(body_mods(fam) + [nn.Linear(H, head)])).to(dev)

    def make(mode):
        fam, kind = mode.rsplit("_", 1)
        env = formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device=dev)
        env.seed(1)
        venv = FormationVecEnv(env, reset_mode="device")
        venv.reset()
        env.world.step_count.copy_((torch.arange(B, device=dev) % 100).int())     # episodes end at different steps
        state = dict(rnn_state=torch.zeros(B, N, H, device=dev)) if fam == "gru" else {}
        if kind == "captured":
            logits = net(fam, 5)
            table = torch.tensor([[0, 0], [-1, 0], [1, 0], [0, -1], [0, 1]], dtype=torch.float32, device=dev)
            h = torch.zeros(B, N, H, device=dev)

            def policy(o):
                if fam == "gru":
                    lg, hn = logits(o, h)
                    h.copy_(hn)
                else:
                    lg = logits(o)
                cdf = torch.softmax(lg, -1).cumsum(-1)[..., :4]
                return table[(torch.rand_like(cdf[..., :1]) >= cdf).sum(-1)]
            with torch.no_grad():
                return venv.capture(policy, K).replay
        if kind == "cat":
            env.discrete_action_input = True
            actor = formation_gym.CategoricalActor(net(fam, 5))
        else:
            actor = formation_gym.GaussianActor(net(fam, 2), nn.Parameter(torch.full((2,), -0.5, device=dev)))
        assert env.actor_path(actor) == "fused", mode
        return lambda: env.rollout_actor(K, actor, **state)

    bodies, reps = {}, {}
    for mode in modes:
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
    blocks = {mode: [] for mode in modes}
    for _ in range(ROUNDS):
        for mode in modes:                                                       # the variants alternate
            body = bodies[mode]
            t0 = time.perf_counter()
            for _ in range(reps[mode]):
                body()
            torch.cuda.synchronize()
            blocks[mode].append((time.perf_counter() - t0) / (reps[mode] * K) * 1e6)
    return {("parent_" if parent else "") + mode: v for mode, v in blocks.items()}


def child(N, B, lib):
    r = subprocess.run([sys.executable, __file__, "--one", str(N), str(B), str(H)] + ([lib] if lib else []), capture_output=True,
                       text=True, timeout=900)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[:4000] + "\n...\n" + r.stderr[-1000:])
        raise SystemExit("%d x %d failed (%d)" % (N, B, r.returncode))
    out = {}
    for line in r.stdout.splitlines():
        f = line.split()
        if len(f) >= 2 and f[0].rsplit("_", 1)[-1] in ("cat", "gauss", "captured"):
            out[f[0]] = [float(x) for x in f[1:]]
    return out


def main(parent_lib):
    for N, B in SHAPES:
        t = {}
        for _ in range(OUTER):                                                   # the libraries' children alternate
            for lib in ([None, parent_lib] if parent_lib else [None]):
                for mode, v in child(N, B, lib).items():
                    t.setdefault(mode, []).extend(v)
        print("\n%d x %d, H = %d, K = %d: us per env step, median (min - max)\n" % (N, B, H, K))
        print("| family | categorical | Gaussian | Gaussian, parent library | captured torch loop | cat / Gaussian | cat / captured |")
        print("|---|---|---|---|---|---|---|")
        cell = lambda v: "%.2f (%.2f - %.2f)" % (statistics.median(v), min(v), max(v)) if v else "-"
        for fam in FAMILIES:
            c, g, p, cap = (t.get(k) for k in (fam + "_cat", fam + "_gauss", "parent_" + fam + "_gauss", fam + "_captured"))
            print("| %s | %s | %s | %s | %s | %.3f | %.2f |" % (fam, cell(c), cell(g), cell(p), cell(cap),
                                                               statistics.median(c) / statistics.median(g),
                                                               statistics.median(c) / statistics.median(cap)), flush=True)


if __name__ == "__main__":
    if len(sys.argv) >= 5 and sys.argv[1] == "--one":
        for mode, v in one(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5] if len(sys.argv) > 5 else None).items():
            print(mode, " ".join("%.4f" % x for x in v))
    else:
        main(sys.argv[2] if len(sys.argv) == 3 and sys.argv[1] == "--parent-lib" else None)
