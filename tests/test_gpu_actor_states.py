"""GPU tests of `env.rollout_actor(K, actor, rnn_state=h, rnn_states_every=S)`: the recurrent launch
(`fg_rollout_hd_actor_gru_states`, gru_actor_kernel / gru_sample_kernel) also keeps the hidden state every S-th step acted with -
onpolicy's rnn_states[step], what rMAPPO's recurrent generator restarts each data chunk from.

The kept states are not a new computation: entry j is the state block the launch already carries, copied out before step j S
reads it.  So the checks are equalities, bit for bit - against the `rnn_state` tensor going into each of K one-step calls (which
test_gpu_actor_recurrent.py holds to the fp64 actor), across splits of K, across strides, and of everything else the launch
returns against the launch that keeps nothing.

Shapes.  B = 133 leaves a tail workgroup at every workgroup size, K = 24, a third of the envs end an episode at step 7.  A
workgroup's rows are stored in wave passes of 32: N = 3 (64 envs x 3 = 192 rows) has whole passes, N = 9 (144 rows) a half-full
last pass, N = 27 (216 rows) a three-quarters one; H = 64 and, at N = 9, H = 32.  A random non-zero initial state.  Every test
runs the deterministic and the Gaussian kernel.

Host-paced twin.  The same modules with the base behind `Wrap` run the loop in Python, which keeps `h.clone()` before the actor
call.  The two paths hold the same fp32 state only until the first step, so entry 0 is compared exactly and entry 1 within
twice test_gpu_actor_recurrent.py's state bound, 2 TOL max(1, r1) max(1, r2) (both sides carry it; tests/actor_fidelity.py).
Largest measured diff / (2 bound) of entry 1 on MI355X (lines starting STATESTWIN, printed before the assertion): 0.0193
at (N, H) = (27, 64); (3, 64) 0.0153, (9, 64) 0.0082, (9, 32) 0.0071, the same for the deterministic and the Gaussian kernel
(the noise is added after the state is written).
"""
import copy

import pytest
import torch

from formation_gym import GaussianActor, RecurrentActor, _native
from tests.actor_fidelity import EDGE_EPS, TOL, rec_actor, rec_ref64
from tests.actor_testlib import (B, DEV, K, Wrap, clone as _clone, current_obs as _current_obs, env as _env, state as _state)

pytestmark = pytest.mark.gpu

nn = torch.nn
SHAPES = [(3, 64), (9, 64), (27, 64), (9, 32)]
CASES = [(n, h, g) for n, h in SHAPES for g in (False, True)]
_IDS = ["N%d-H%d-%s" % (n, h, "gauss" if g else "det") for n, h, g in CASES]
cases = pytest.mark.parametrize("N,H,gaussian", CASES, ids=_IDS)


def _random_state(N, H, seed=11):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((B, N, H), generator=g) * 2 - 1).to(DEV)


def _make_actor(N, H, gaussian, eps=1e-5):
    mean = rec_actor(N, H, in_norm=(N != 9), tanh=(H == 64), eps=eps, device=DEV)
    return GaussianActor(mean, nn.Parameter(torch.tensor([-0.5, 0.3], device=DEV))) if gaussian else mean


def _twin(actor):
    """The same modules, the base behind a module the path rule does not recognise: runs host-paced."""
    mean = actor.mean if isinstance(actor, GaussianActor) else actor
    host = RecurrentActor(Wrap(mean.base), mean.rnn, mean.norm, mean.head)
    return GaussianActor(host, actor.log_std) if isinstance(actor, GaussianActor) else host


_SHARED = {}


def _setup(N, H, gaussian):
    """(env, actor, h0, snapshot, the S = 1 launch from it): built once per case and left unchanged; the env is handed back
    restored to the snapshot."""
    key = (N, H, gaussian)
    if key not in _SHARED:
        env = _env(N)
        actor = _make_actor(N, H, gaussian)
        assert env.actor_path(actor) == "fused"
        h0 = _random_state(N, H)
        snap = env._snapshot()
        h = h0.clone()
        res = _clone(env.rollout_actor(K, actor, rnn_state=h, rnn_states_every=1))
        assert res[3]["rnn_states"].shape == (K, B, N, H) and res[3]["rnn_states"].dtype == torch.float32
        assert res[3]["rnn_states"].is_contiguous() and res[3]["rnn_states"].device == h.device
        assert bool(res[2].any()), "no episode boundary inside the launch"
        _SHARED[key] = (env, actor, h0, snap, res)
    env, actor, h0, snap, res = _SHARED[key]
    env._restore(snap)
    env.auto_reset = True
    return env, actor, h0, snap, res


def _states_of_one_step_calls(env, actor, h0, steps):
    """The `rnn_state` tensor going into each of `steps` one-step calls that pass the state along."""
    h, seen = h0.clone(), []
    for _ in range(steps):
        seen.append(h.clone())
        env.rollout_actor(1, actor, rnn_state=h)
    return torch.stack(seen), h


def _split_and_stride(env, actor, h0, snap, every_step):
    """Tests 1 and 2 of one path (fused or host-paced) against itself; `every_step`: its S = 1 entries [K, B, N, *]."""
    assert torch.equal(every_step[0], h0)
    env._restore(snap)
    seen, h_end = _states_of_one_step_calls(env, actor, h0, K)
    assert torch.equal(seen, every_step), "S = 1 entries differ from the states going into K one-step calls"
    for S in (1, 5):                                             # one 10 + 14 split: steps 0, 5 | 10, 15, 20 at S = 5
        env._restore(snap)
        h = h0.clone()
        first = env.rollout_actor(10, actor, rnn_state=h, rnn_states_every=S)[3]["rnn_states"].clone()
        second = env.rollout_actor(14, actor, rnn_state=h, rnn_states_every=S)[3]["rnn_states"].clone()
        assert torch.equal(torch.cat((first, second)), every_step[::S])
        assert torch.equal(h, h_end)
    for S, steps in ((5, [0, 5, 10, 15, 20]), (24, [0]), (30, [0])):
        env._restore(snap)
        h = h0.clone()
        got = env.rollout_actor(K, actor, rnn_state=h, rnn_states_every=S)[3]["rnn_states"]
        assert got.shape == (len(steps),) + tuple(h0.shape)
        assert torch.equal(got, every_step[steps]), "S = %d" % S
        assert torch.equal(h, h_end)


@cases
def test_split_equality_and_stride(N, H, gaussian):
    env, actor, h0, snap, ref = _setup(N, H, gaussian)
    _split_and_stride(env, actor, h0, snap, ref[3]["rnn_states"])


@pytest.mark.parametrize("auto_reset", [True, False])
@cases
def test_masking(N, H, gaussian, auto_reset):
    env, actor, h0, snap, ref = _setup(N, H, gaussian)
    if auto_reset:
        done, states = ref[2], ref[3]["rnn_states"]
    else:
        env.auto_reset = False
        _, _, done, info = env.rollout_actor(K, actor, rnn_state=h0.clone(), rnn_states_every=1)
        states = info["rnn_states"]
    assert bool(done.any()) and bool((~done).any())
    ended, after = done[:-1], states[1:]                         # done[k] [B, N] against rnn_states[k + 1] [B, N, H]
    assert bool((done == done[:, :, :1]).all())
    assert not bool(after[ended].any()), "a state kept after an episode's last step is not exactly zero"
    assert bool((after[~ended] != 0).any(-1).all()), "a row that lives on was kept as zeros"
    assert torch.equal(states[0], h0)


@pytest.mark.parametrize("obs_every", [1, 5])
@cases
def test_nothing_else_moves(N, H, gaussian, obs_every):
    env, actor, h0, snap, ref = _setup(N, H, gaussian)
    h_plain = h0.clone()
    plain = _clone(env.rollout_actor(K, actor, obs_every=obs_every, rnn_state=h_plain))
    plain_state = _state(env)
    assert "rnn_states" not in plain[3]
    env._restore(snap)
    h_rec = h0.clone()
    rec = _clone(env.rollout_actor(K, actor, obs_every=obs_every, rnn_state=h_rec, rnn_states_every=1 if obs_every == 1 else 5))
    assert plain[0].shape[0] == K // obs_every
    for a, b in zip(plain[:3], rec[:3]):                         # observations, rewards, done flags
        assert torch.equal(a, b)
    assert set(rec[3]) == set(plain[3]) | {"rnn_states"} and ("log_prob" in plain[3]) == gaussian
    for k in plain[3]:                                           # actions, individual rewards, log-probs, the final state
        assert torch.equal(plain[3][k], rec[3][k]), k
    assert torch.equal(h_plain, h_rec) and not torch.equal(h_rec, h0)
    for a, b in zip(plain_state, _state(env)):
        assert torch.equal(a, b)
    if obs_every == 1:                                           # and the shared launch is that launch
        for a, b in zip(rec[:3], ref[:3]):
            assert torch.equal(a, b)
        assert torch.equal(rec[3]["rnn_states"], ref[3]["rnn_states"])


@cases
def test_host_paced_twin(N, H, gaussian):
    env, actor, h0, snap, ref = _setup(N, H, gaussian)
    host = _twin(actor)
    assert env.actor_path(host) == "host"
    obs0 = _current_obs(env)
    h = h0.clone()
    _, _, h_done, h_info = _clone(env.rollout_actor(K, host, rnn_state=h, rnn_states_every=1))
    h_states = h_info["rnn_states"]
    assert h_states.shape == (K, B, N, H) and h_states.dtype == torch.float32 and h_states.is_contiguous()
    _split_and_stride(env, host, h0, snap, h_states)
    # against the fused launch: entry 0 is the state passed in on both sides, entry 1 one fp32 step of either away from it
    f_states, f_done = ref[3]["rnn_states"], ref[2]
    assert torch.equal(f_states[0], h_states[0])
    assert torch.equal(f_done[0], h_done[0]) and torch.equal(f_states[1] == 0, h_states[1] == 0)
    mean = actor.mean if gaussian else actor
    with torch.no_grad():
        _, _, r1, r2, _ = rec_ref64(copy.deepcopy(mean).double(), obs0.double(), h0.double())
    bound = 2 * TOL * torch.clamp(r1, min=1.0) * torch.clamp(r2, min=1.0)
    ratio = float(((f_states[1].double() - h_states[1].double()).abs() / bound).max())
    print("STATESTWIN N=%d H=%d gaussian=%d entry 1, max diff/(2 bound) = %.4f" % (N, H, gaussian, ratio))
    assert ratio <= 1.0


@pytest.mark.parametrize("gaussian", [False, True])
def test_two_layer_gru_member_keeps_both_layers(gaussian):
    N, H = 9, 64
    env = _env(N)
    mean = rec_actor(N, H, True, device=DEV)
    mean.rnn = nn.GRU(H, H, num_layers=2).to(DEV)
    actor = GaussianActor(mean, nn.Parameter(torch.zeros(2, device=DEV))) if gaussian else mean
    assert env.actor_path(actor) == "host" and mean.state_size == 2 * H
    h0 = _random_state(N, 2 * H)
    h = h0.clone()
    _, _, done, info = env.rollout_actor(8, actor, rnn_state=h, rnn_states_every=7)      # steps 0 and 7; step 6 ends episodes
    assert info["rnn_states"].shape == (2, B, N, 2 * H) and torch.equal(info["rnn_states"][0], h0)
    assert bool(done[6].any()) and not bool(info["rnn_states"][1][done[6]].any())
    assert bool((info["rnn_states"][1][~done[6]] != 0).any(-1).all())


def _out(N, steps, gaussian, S, H):
    f = dict(dtype=torch.float32, device=DEV)
    out = dict(obs=torch.empty((steps, B, N, 6 * N), **f), reward=torch.empty((steps, B, N), **f),
               indiv=torch.empty((steps, B, N), **f), done=torch.zeros((steps, B, N), dtype=torch.uint8, device=DEV),
               act=torch.empty((steps, B, N, 2), **f), rnn_states=torch.zeros(((steps + S - 1) // S, B, N, H), **f))
    if gaussian:
        out["log_prob"] = torch.empty((steps, B, N), **f)
    return out


@pytest.mark.parametrize("gaussian", [False, True])
def test_buffers_and_errors(gaussian):
    N, H, S = 9, 64, 5
    env, actor, h0, snap, ref = _setup(N, H, gaussian)
    want = ref[3]["rnn_states"][::S]
    env._roll_launchers.clear()
    # a caller's tensor is written in place and handed back
    out = _out(N, K, gaussian, S, H)
    info = env.rollout_actor(K, actor, out=out, rnn_state=h0.clone(), rnn_states_every=S)[3]
    assert info["rnn_states"] is out["rnn_states"] and torch.equal(out["rnn_states"], want)
    assert len(env._roll_launchers) == 1
    # the same buffers and state: the bound launcher again; another states tensor: a launcher of its own, writing there
    env._restore(snap)
    h = h0.clone()
    env.rollout_actor(K, actor, out=out, rnn_state=h, rnn_states_every=S)
    bound = dict(env._roll_launchers)
    env._restore(snap)
    h.copy_(h0)
    out["rnn_states"].zero_()
    env.rollout_actor(K, actor, out=out, rnn_state=h, rnn_states_every=S)
    assert dict(env._roll_launchers) == bound and torch.equal(out["rnn_states"], want)
    other = dict(out, rnn_states=torch.zeros_like(out["rnn_states"]))
    env._restore(snap)
    h.copy_(h0)
    out["rnn_states"].zero_()
    info = env.rollout_actor(K, actor, out=other, rnn_state=h, rnn_states_every=S)[3]
    assert len(env._roll_launchers) == len(bound) + 1, "a launcher bound with one states tensor was reused for another"
    assert info["rnn_states"] is other["rnn_states"] and torch.equal(other["rnn_states"], want)
    assert not bool(out["rnn_states"].any())
    # what the launch cannot take
    good = out["rnn_states"]
    wide = torch.zeros((good.shape[0], B, N, 2 * H), device=DEV)
    for bad in (good[:-1].clone(), wide[..., ::2], good.double(), good.cpu(), torch.zeros((good.shape[0], B, N, 32), device=DEV)):
        assert bad.shape != good.shape or not bad.is_contiguous() or bad.dtype != good.dtype or bad.device != good.device
        with pytest.raises(ValueError):
            env.rollout_actor(K, actor, out=dict(out, rnn_states=bad), rnn_state=h0.clone(), rnn_states_every=S)
    for bad_s in (0, -1, 2.5, True):
        with pytest.raises(ValueError):
            env.rollout_actor(K, actor, rnn_state=h0.clone(), rnn_states_every=bad_s)
    mean = actor.mean if gaussian else actor
    plain = nn.Sequential(*mean.base, nn.Linear(H, 2).to(DEV))
    plain = GaussianActor(plain, actor.log_std) if gaussian else plain
    assert env.actor_path(plain) == "fused"
    with pytest.raises(ValueError):
        env.rollout_actor(K, plain, rnn_states_every=S)
    # out=None: kept with the shape's env-owned buffers, replaced when S changes; out=False: fresh
    env._restore(snap)
    first = env.rollout_actor(K, actor, rnn_state=h0.clone(), rnn_states_every=S)[3]["rnn_states"]
    assert torch.equal(first, want)
    env._restore(snap)
    again = env.rollout_actor(K, actor, rnn_state=h0.clone(), rnn_states_every=S)[3]["rnn_states"]
    assert again.data_ptr() == first.data_ptr() and again.shape == first.shape
    env._restore(snap)
    every = env.rollout_actor(K, actor, rnn_state=h0.clone(), rnn_states_every=1)[3]["rnn_states"]
    assert every.data_ptr() != first.data_ptr() and every.shape == (K, B, N, H)
    assert torch.equal(every, ref[3]["rnn_states"])
    env._restore(snap)
    fresh = [env.rollout_actor(3, actor, out=False, rnn_state=h0.clone(), rnn_states_every=1)[3]["rnn_states"] for _ in (0, 1)]
    assert fresh[0].data_ptr() != fresh[1].data_ptr()
    # and without the keyword: today's call
    env._restore(snap)
    assert "rnn_states" not in env.rollout_actor(K, actor, rnn_state=h0.clone())[3]


def test_c_abi_call_equals_rollout_actor():
    N, H, S = 9, 64, 5
    env = _env(N)
    mean = rec_actor(N, H, True, tanh=True, eps=EDGE_EPS, device=DEV)      # one eps per norm: the fields cannot be permuted
    log_std = nn.Parameter(torch.tensor([0.2, -0.4], device=DEV))
    actor = GaussianActor(mean, log_std)
    assert env.actor_path(actor) == "fused"
    h0 = _random_state(N, H)
    snap = env._snapshot()
    h = h0.clone()
    obs, rew, done, info = _clone(env.rollout_actor(K, actor, rnn_state=h, rnn_states_every=S))
    state = _state(env)
    env._restore(snap)
    o = _out(N, K, True, S, H)
    lins = [m for m in mean.base if isinstance(m, nn.Linear)] + [mean.head[0]]
    lns = [m for m in mean.base if isinstance(m, nn.LayerNorm)]
    fa = _native.FgActor(H, 1, *[t.data_ptr() for l in lins for t in (l.weight, l.bias)])
    fn = _native.FgActorNorm(lns[0].weight.data_ptr(), lns[0].bias.data_ptr(), lns[1].weight.data_ptr(), lns[1].bias.data_ptr(),
                             lns[2].weight.data_ptr(), lns[2].bias.data_ptr(), lns[0].eps, lns[1].eps, lns[2].eps, 1)
    g = mean.rnn
    fgru = _native.FgActorGru(g.weight_ih.data_ptr(), g.weight_hh.data_ptr(), g.bias_ih.data_ptr(), g.bias_hh.data_ptr(),
                              mean.norm.weight.data_ptr(), mean.norm.bias.data_ptr(), mean.norm.eps)
    hc = h0.clone()
    w, sc = env.world, env.scenario
    p = sc.params(w, True, env._launch_rng_offset(), o["obs"])
    rc = _native.load().fg_rollout_hd_actor_gru_states(
        p, fa, fn, fgru, log_std.data_ptr(), B, N, K, w.pos_x.data_ptr(), w.pos_y.data_ptr(),
        w.vel_x.data_ptr(), w.vel_y.data_ptr(), o["act"].data_ptr(), sc.ideal_shape.data_ptr(), sc.ideal_vel.data_ptr(),
        w.step_count.data_ptr(), o["obs"].data_ptr(), o["reward"].data_ptr(), o["indiv"].data_ptr(), o["done"].data_ptr(),
        o["log_prob"].data_ptr(), hc.data_ptr(), o["rnn_states"].data_ptr(), S, 1, _native.current_stream(DEV))
    _native.check(rc)
    torch.cuda.synchronize()
    assert torch.equal(o["rnn_states"], info["rnn_states"]) and torch.equal(o["rnn_states"][0], h0)
    assert torch.equal(o["act"], info["actions"]) and torch.equal(o["obs"], obs)
    assert torch.equal(o["indiv"], info["individual_reward"]) and torch.equal(o["done"].view(torch.bool), done)
    assert torch.equal((o["reward"] if env.shared_reward else o["indiv"]).unsqueeze(-1), rew)
    assert torch.equal(o["log_prob"], info["log_prob"])
    assert torch.equal(hc, h)
    for a, b in zip(state, _state(env)):
        assert torch.equal(a, b)
