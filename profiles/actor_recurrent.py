#!/usr/bin/env python3
"""The exploring loop of rMAPPO's recurrent actor (onpolicy's R_Actor: MLPBase - GRU - LayerNorm - DiagGaussian), us per env
step (K = 20 steps per call):

  gru        env.rollout_actor(K, GaussianActor(RecurrentActor(base, GRUCell, LayerNorm, head), log_std), rnn_state=h): ONE
             gru_sample_kernel launch (fg_rollout_hd_actor_gru), the hidden state in LDS for the whole launch
  gru_s1     ... with rnn_states_every=1 (fg_rollout_hd_actor_gru_states): the same launch also stores the state every step
  gru_s10    acted with / every tenth step acted with, B N H 4 bytes per kept step
  ln         env.rollout_actor(K, GaussianActor(Sequential(*base, head), log_std)): the same body and head without the
             recurrent layer, ln_sample_kernel, for the cost of the GRU and its norm
  captured   FormationVecEnv.capture(policy, K) with the host-paced recurrent loop as the policy -
             h *= (step_count != 0); mu, h = actor(o, h); a = mu + exp(log_std) * randn - captured once in a hipGraph
             (torch.cuda.graph) and replayed

base = Sequential(LayerNorm(6N), Linear(6N, H), ReLU, LayerNorm(H), Linear(H, H), ReLU, LayerNorm(H)), head = Linear(H, 2),
log_std = -0.5.  Every measurement runs in a process of its own (`--one MODE N B H`): ~1 s of the same work to warm the clocks,
then the median of 7 timed blocks.
Usage:  python3 profiles/actor_recurrent.py [N B ...]     (the table, markdown on stdout; default 9 4096 27 4096)
        python3 profiles/actor_recurrent.py --states [--lib OTHER.so] [N B ...]
            the cost of keeping the states: REPS rounds of (OTHER.so's gru,) gru, gru_s1, gru_s10, interleaved, one process
            each; per configuration every round's figure, their median and spread, and for the keeping launches the added
            us/step and the bytes of state written over the added time.  OTHER.so: libformation_hip.so of another commit (the
            parent's, to see what the run-time branch costs the launch that keeps nothing), driven by this tree's Python.
Kernel time: rocprofv3 --kernel-trace --stats -- python3 profiles/actor_recurrent.py --one gru 9 4096 64  (and ln)."""
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
MODES = ("gru", "ln", "captured")
REPS = 5
KEEP = {"gru_s1": 1, "gru_s10": 10}


def one(mode, N, B, H, lib=None):
    import torch
    import formation_gym
    if lib is not None:                                  # another commit's library: bind what it exports
        from formation_gym import _native
        _native.LIB_PATH = os.path.abspath(lib)
        import ctypes
        have = ctypes.CDLL(_native.LIB_PATH)
        for name in [n for n in _native.SIGNATURES if not hasattr(have, n)]:
            del _native.SIGNATURES[name]
    from formation_gym.vec_env import FormationVecEnv
    nn = torch.nn
    dev = "cuda:0"
    torch.manual_seed(0)
    D = 6 * N
    base = nn.Sequential(nn.LayerNorm(D), nn.Linear(D, H), nn.ReLU(), nn.LayerNorm(H), nn.Linear(H, H), nn.ReLU(), nn.LayerNorm(H))
    head = nn.Linear(H, 2)
    rec = formation_gym.RecurrentActor(base, nn.GRUCell(H, H), nn.LayerNorm(H), head).to(dev)
    log_std = nn.Parameter(torch.full((2,), -0.5, device=dev))
    env = formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device=dev)
    env.seed(1)
    venv = FormationVecEnv(env, reset_mode="device")
    venv.reset()
    env.world.step_count.copy_((torch.arange(B, device=dev) % 100).int())     # episodes end at different steps
    h = rec.initial_state(B, N)
    if mode == "gru":
        actor = formation_gym.GaussianActor(rec, log_std)
        assert env.actor_path(actor) == "fused"
        body = lambda: env.rollout_actor(K, actor, rnn_state=h)                  # noqa: E731
    elif mode in KEEP:
        actor = formation_gym.GaussianActor(rec, log_std)
        assert env.actor_path(actor) == "fused"
        body = lambda: env.rollout_actor(K, actor, rnn_state=h, rnn_states_every=KEEP[mode])   # noqa: E731
    elif mode == "ln":
        actor = formation_gym.GaussianActor(nn.Sequential(*base, head), log_std)
        assert env.actor_path(actor) == "fused"
        body = lambda: env.rollout_actor(K, actor)                               # noqa: E731
    else:
        for q in list(rec.parameters()) + [log_std]:
            q.requires_grad_(False)                                              # a rollout: no autograd graph through h

        def policy(o):
            h.mul_((env.world.step_count != 0)[:, None, None])                   # a fresh episode starts from zeros
            mu, hn = rec(o, h)
            h.copy_(hn)
            return mu + torch.exp(log_std) * torch.randn_like(mu)
        with torch.no_grad():
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


def main(shapes):
    print("| shape | H | gru us/step | ln us/step | captured recurrent loop us/step | gru / ln | gru / captured |")
    print("|---|---|---|---|---|---|---|")
    for N, B in shapes:
        for H in HIDDEN:
            t = {}
            for mode in MODES:
                t[mode] = _run_one(mode, N, B, H)
            print("| %d x %d | %d | %.2f | %.2f | %.2f | %.3f | %.2f |" % (
                N, B, H, t["gru"], t["ln"], t["captured"], t["gru"] / t["ln"], t["gru"] / t["captured"]), flush=True)


def _run_one(mode, N, B, H, lib=None):
    cmd = [sys.executable, __file__, "--one", mode, str(N), str(B), str(H)] + ([lib] if lib else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-2000:])
        raise SystemExit("%s %d x %d H %d failed (%d)" % (mode, N, B, H, r.returncode))
    return float(r.stdout.strip().split()[-1])


def states(shapes, lib):
    configs = ([("other gru", "gru", lib)] if lib else []) + [("gru", "gru", None), ("gru_s1", "gru_s1", None),
                                                                ("gru_s10", "gru_s10", None)]
    print("| shape | H | configuration | us/step per round | median | min - max | added us/step | state bytes per call | GB/s of"
          " state over the added time |")
    print("|---|---|---|---|---|---|---|---|---|")
    for N, B in shapes:
        for H in HIDDEN:
            t = {name: [] for name, _, _ in configs}
            for _ in range(REPS):                        # interleaved: a drift of the machine reaches every configuration
                for name, mode, other in configs:
                    t[name].append(_run_one(mode, N, B, H, other))
            base = statistics.median(t["gru"])
            for name, mode, _ in configs:
                med = statistics.median(t[name])
                cost = "| | | |"
                if mode in KEEP:
                    nbytes = -(-K // KEEP[mode]) * B * N * H * 4
                    added = med - base
                    cost = "| %+.3f | %.1f MB | %s |" % (added, nbytes / 1e6,
                                                         "%.0f" % (nbytes / (added * K * 1e-6) / 1e9) if added > 0 else "-")
                print("| %d x %d | %d | %s | %s | %.3f | %.3f - %.3f (%.1f %%) %s" % (
                    N, B, H, name, " ".join("%.3f" % x for x in t[name]), med, min(t[name]), max(t[name]),
                    100.0 * (max(t[name]) - min(t[name])) / med, cost), flush=True)


if __name__ == "__main__":
    if len(sys.argv) in (6, 7) and sys.argv[1] == "--one":
        print("%.4f" % one(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]), *sys.argv[6:7]))
    elif len(sys.argv) > 1 and sys.argv[1] == "--states":
        rest = sys.argv[2:]
        other = None
        if rest[:1] == ["--lib"]:
            other, rest = rest[1], rest[2:]
        nums = [int(x) for x in rest]
        states(tuple(zip(nums[0::2], nums[1::2])) or SHAPES, other)
    else:
        nums = [int(x) for x in sys.argv[1:]]
        main(tuple(zip(nums[0::2], nums[1::2])) or SHAPES)
