"""Multi-device tests: everything here needs TWO visible GPUs and is skipped on a one-GPU box.

What they pin (VERDICT r2 item 1c / ADVICE r2): a launch goes to the device its data lives on - also on the NULL
(default) stream, which torch hands out as handle 0 for every device - so an env on cuda:1 can be driven from a thread
whose current device is cuda:0; the per-device bookkeeping of the > 64 KiB dynamic-LDS opt-in of the pipelined rollout
kernels; one process driving two devices from two threads; two rank processes on distinct devices with the RCCL
timing barrier.  Environments never interact, so every comparison is bit for bit against a cuda:0 run.
"""
import threading

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs")]


def _make(N, B, device, seed=3):
    import formation_gym
    env = formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device=device)
    env.seed(seed)
    env.reset()
    env.auto_reset = True
    env.world.step_count.copy_((torch.arange(B, dtype=torch.int32) * 13 % 100).to(device))
    return env


def _drive(env, N, B, K, seed=11):
    """One single step, one K-step rollout (the pipelined kernels: 92 KB of dynamic LDS at 27 agents), one more
    single step; everything returned on the host."""
    dev = env.world.device
    gen = torch.Generator(); gen.manual_seed(seed)
    acts = (torch.rand((K + 2, B, N, 2), generator=gen) * 2 - 1).to(dev)
    res = []
    o, r, d, i = env.step(acts[0])
    res += [o.cpu().clone(), r.cpu().clone(), d.cpu().clone(), i["individual_reward"].cpu().clone()]
    o, r, d, i = env.rollout(acts[1:K + 1].contiguous())
    res += [o.cpu(), r.cpu(), d.cpu(), i["individual_reward"].cpu()]
    o, r, d, i = env.step(acts[K + 1])
    res += [o.cpu().clone(), r.cpu().clone(), d.cpu().clone()]
    pos, vel = env.world.get_state()
    res += [pos.cpu(), vel.cpu(), env.scenario.ideal_shape.cpu().clone(), env.world.step_count.cpu().clone()]
    return res


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("N,B,K", [(27, 96, 6), (9, 200, 5), (81, 24, 3), (10, 33, 4)])
def test_env_on_second_device_driven_from_a_thread_on_the_first(N, B, K):
    """The default stream of cuda:1 is handle 0, like cuda:0's: the library must read the device off the data."""
    torch.cuda.set_device(0)
    want = _drive(_make(N, B, "cuda:0"), N, B, K)
    env1 = _make(N, B, "cuda:1")
    assert torch.cuda.current_device() == 0
    got = _drive(env1, N, B, K)
    assert torch.cuda.current_device() == 0            # the library restores the caller's device
    torch.cuda.synchronize(1)
    _same(got, want)
    # ... and on a non-default stream of cuda:1, still from a cuda:0 thread
    env1b = _make(N, B, "cuda:1")
    s = torch.cuda.Stream(device=1)
    s.wait_stream(torch.cuda.current_stream(1))
    with torch.cuda.stream(s):
        got2 = _drive(env1b, N, B, K)
    torch.cuda.set_device(0)
    _same(got2, want)


def test_other_entry_points_follow_their_data():
    """Controller, device resets (counter RNG and MT19937), landmark scenarios, action decoding on cuda:1 from cuda:0."""
    import formation_gym
    from formation_gym.vec_env import FormationVecEnv
    torch.cuda.set_device(0)
    out = {}
    for dev in ("cuda:0", "cuda:1"):
        res = []
        env = _make(27, 64, dev)
        act = formation_gym.get_action_BFS(formation_gym.ezpolicy, env._out["obs"], 3)
        res.append(act.cpu().clone())
        o, r, d, i = env.rollout_policy(5, 3)
        res += [o.cpu(), r.cpu(), i["actions"].cpu()]
        env.scenario.reset_device(env.world, rng_offset=77)
        res.append(env.world.pos_x.cpu().clone())
        v = FormationVecEnv(_make(9, 50, dev), reset_mode="device_mt")
        res.append(v.reset().cpu().clone())
        for t in range(3):
            o, r, d, i = v.step(torch.full((50, 9, 2), 0.1 * (t + 1), device=dev))
        res.append(o.cpu().clone())
        e2 = formation_gym.make_env("formation_hd_obs_env", False, 4, num_envs=32, device=dev)
        e2.seed(2); e2.reset()
        o, r, d, i = e2.step(torch.full((32, 4, 2), 0.3, device=dev))
        res += [o.cpu().clone(), r.cpu().clone()]
        out[dev] = res
        assert torch.cuda.current_device() == 0
    _same(out["cuda:1"], out["cuda:0"])


def test_two_threads_of_one_process_drive_two_devices():
    """One thread per GPU, each with its own current device, launching concurrently (re-entrant C ABI, per-device
    LDS opt-in recorded atomically): both reproduce the single-threaded cuda:0 results."""
    N, B, K = 27, 128, 8
    torch.cuda.set_device(0)
    want = _drive(_make(N, B, "cuda:0"), N, B, K)
    results, errors = {}, []

    def worker(idx):
        try:
            torch.cuda.set_device(idx)
            env = _make(N, B, "cuda:%d" % idx)
            for _ in range(3):                         # several rounds: launches of both threads interleave
                env2 = _make(N, B, "cuda:%d" % idx)
                results[idx] = _drive(env2, N, B, K)
            del env
        except Exception as exc:                       # noqa: BLE001 - reported by the main thread
            errors.append((idx, repr(exc)))

    threads = [threading.Thread(target=worker, args=(i,)) for i in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=300)
    assert not errors, errors
    for idx in (0, 1):
        _same(results[idx], want)


def test_two_rank_processes_on_distinct_devices_with_the_rccl_barrier(tmp_path):
    """torch.distributed.run with one rank per GPU: the shards reproduce the one-process batch bit for bit, and
    bench.py brings up its RCCL timing group (backend "nccl") when every rank has its own device."""
    import json
    from tests.test_gpu_parity import _free_port, _run
    from formation_gym import sharding
    N, G, K = 9, 37, 12
    torch.cuda.set_device(0)
    whole, lo, hi = sharding.make_env_shard("formation_hd_env", N, G, seed=5, rank=0, world_size=1, local_rank=0)
    whole.auto_reset = True
    whole.reset()
    whole.world.step_count.copy_((torch.arange(G, dtype=torch.int32) * 7 % 100).cuda())
    gen = torch.Generator(); gen.manual_seed(123)
    acts = (torch.rand((K, G, N, 2), generator=gen) * 2 - 1).cuda()
    obs, rew, done, info = whole.rollout(acts)
    out = str(tmp_path / "shards_2dev.npz")
    _run(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
          "--master-port", _free_port(), "tests/helpers/shard_worker.py", out, str(N), str(G), str(K)],
         env_extra={"HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    r = np.load(out)
    np.testing.assert_array_equal(r["obs_last"], obs[-1].cpu().numpy())
    np.testing.assert_array_equal(r["rew"], rew[..., 0].permute(1, 0, 2).cpu().numpy())
    np.testing.assert_array_equal(r["pos_x"], whole.world.pos_x.cpu().numpy())
    line = [l for l in _run(["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                             "127.0.0.1", "--master-port", _free_port(), "bench.py", "--gpus", "2", "--steps", "20",
                             "--warmup", "5", "--envs", "512", "--agents", "27", "--full", "--no-cpu-baseline", "--global-div", "32",
                             "--min-timed-ms", "5"], env_extra={"HSA_ENABLE_IPC_MODE_LEGACY": "0"},
                            timeout=600).splitlines() if l.startswith("{")]
    assert len(line) == 1
    d = json.loads(line[0])
    assert d["n_gpus"] == 2 and d["config"]["timing_barrier"] == "rccl" and d["state_finite"]
    for g in d["global_configs"]:
        assert len(g["per_rank_ms_per_step"]) == 2 and g["state_finite"]
        assert g["n1_same_run"] and 0.2 < g["scaling_efficiency_vs_n1"] < 1.5


def test_placed_buffers_on_the_second_device():
    """env.alloc_rollout_buffers for an env on cuda:1 from a thread whose current device is cuda:0: the arena is made on
    the env's device (fg_arena_create(device = 1)), and a rollout into the placed buffer equals step calls."""
    from formation_gym import placement
    N, B, K = 27, 4096, 8
    torch.cuda.set_device(0)
    a, b = _make(N, B, "cuda:1"), _make(N, B, "cuda:1")
    for e in (a, b):
        e.seed(3); e.reset()
    out = b.alloc_rollout_buffers(K)
    assert torch.cuda.current_device() == 0
    assert out["obs"].device == torch.device("cuda:1") and b.placement["probed"]
    if b.placement.get("kept", "as created") != "as created":
        assert placement.is_placed(out["obs"].data_ptr())
    gen = torch.Generator(device="cuda:1"); gen.manual_seed(1)
    acts = (torch.rand((K, B, N, 2), generator=gen, device="cuda:1") * 2 - 1).contiguous()
    obs, rew, done, info = b.rollout(acts, out=out)
    for k in range(K):
        o, r, d, i = a.step(acts[k])
        assert torch.equal(o, obs[k]) and torch.equal(r, rew[k])
    torch.cuda.synchronize(1)
