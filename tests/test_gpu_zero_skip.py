"""Zero-primed rollout buffers (`FgParams.obs_zero_primed`): the 16-32-agent tile writers leave out the stores of whole
128-byte lines inside the rows' communication block - units [N, 2N-1) of every 3N-unit row, zeros for silent agents - when
the env's own buffer was filled with zeros once (`alloc_rollout_buffers`, placement.register_primed).

* both forms of the tile writer, each case's instantiation confirmed with `fg_describe_launch` - the HBM-streaming one with
  eight writer waves (27 x 2056 = 128 full 16-env workgroups and one of 8 envs; the dispatch streams from 400 MB on, so 12
  steps per launch, not 8: 432 MB) and its four-wave sibling (an ordinary allocation between 3073 and 8191 envs: 27 x 3080 x 8),
  the plain one with 16-env workgroups (27 x 2056 x 2), with 8-env workgroups (27 x 1030 x 3) and with the 2-env small-batch
  geometry (27 x 40 x 5 and 27 x 20 x 5: a full and a half-used writer set) - two consecutive launches into the same primed
  buffer, auto-resets inside, against `env.step` bit for bit;
* a sentinel shows that the skip happens, and only where it may: whole 128-byte lines, by device address, inside one row's block;
* everything that is not the env's own primed fp32 buffer of silent agents runs with the flag at 0.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 27
D = 6 * N
G = 128                                                      # bytes of a skipped group (fg_obs_writers.hpp: FG_ZERO_SKIP_BYTES)
PADDED = -(-6 * N * N // 32) * 32                            # 4384 floats: env blocks padded to whole 128-byte lines


def _make(B):
    import formation_gym
    return formation_gym.make_env("formation_hd_env", False, N, num_envs=B, device="cuda:0")


def _single(B, K2):
    """An env in a device-drawn, crowded state with mixed episode phases: a third of the envs ends its episode inside the
    next K2 steps (at different steps), so that auto-resets fall inside the launches."""
    rs = np.random.RandomState(B)
    step0 = np.where(np.arange(B) % 3 == 0, 100 - 1 - (np.arange(B) // 3) % K2, rs.randint(0, 100 - K2, B))
    e = _make(B)
    e.scenario.seed(3)
    e.scenario.reset_device(e.world, rng_offset=12345)
    e.world.pos_x.mul_(0.45); e.world.pos_y.mul_(0.45)
    e.world.step_count.copy_(torch.as_tensor(step0, dtype=torch.int32))
    e.auto_reset = True
    return e


def _acts(K, B):
    gen = torch.Generator(device="cuda"); gen.manual_seed(K * 100003 + B)
    return (torch.rand((K, B, N, 2), generator=gen, device="cuda") * 2 - 1).contiguous()


def _flag(env, obs):
    return env.scenario.params(env.world, obs=obs).obs_zero_primed


def _registered(env, out):
    """The env keeps a buffer's registration only where the flagged launch measured at least 2 % faster on it than the
    unflagged one (`env.placement["zero_primed"]`), so the buffer is primed here by hand: registered either way."""
    z = env.placement["zero_primed"]
    assert set(z) == {"kept", "flagged_ms", "unflagged_ms"} and z["flagged_ms"] > 0 and z["unflagged_ms"] > 0
    assert _flag(env, out["obs"]) == int(z["kept"])
    env.prime_rollout_buffers(out)
    assert _flag(env, out["obs"]) == 1
    return out


def _describe(env, obs, K):
    """The instantiation `fg_rollout_hd` selects for a K-step launch of this env into `obs`."""
    from formation_gym import _native
    buf = ctypes.create_string_buffer(2048)
    p = env.scenario.params(env.world, auto_reset=True, obs=obs)
    assert _native.load().fg_describe_launch(p, None, env.num_envs, N, K, 0, 1, 0, buf, len(buf)) == 0
    return buf.value.decode().strip()


FORMS = {"stream512": "rollout_kernel<27,32,512,512,16,10,0,1>",     # STREAM form, 8 writer waves (placed, or <= 3072 envs)
         "stream256": "rollout_kernel<27,32,512,256,16,10,0,1>",     # ... its 256-writer-thread sibling
         "plain16": "rollout_kernel<27,32,512,256,16,10,0,0>",       # plain form, 16 envs per workgroup
         "plain8": "rollout_kernel<27,32,256,512,8,10,0,0>",         # ... 8
         "small2": "rollout_kernel<27,32,64,256,2,10,0,0>"}          # ... 2: two writer waves share an env


def _is_form(desc, form):
    assert desc.startswith(FORMS[form] + " "), (form, desc)


# (B, K, obs_every, env pitch, probe candidates, form)
CASES = [(2056, 12, 1, 0, 8, "stream512"),
         (3080, 8, 1, PADDED, 1, "stream256"),       # an ordinary allocation, padded pitch: the written pad, line ownership
         (2056, 2, 1, 0, 8, "plain16"),
         (1030, 3, 1, 0, 8, "plain8"),
         (40, 5, 1, 0, 8, "small2"),
         (40, 6, 2, 0, 8, "small2"),
         (40, 5, 1, PADDED, 8, "small2"),
         (20, 5, 1, 0, 8, "small2")]


@pytest.mark.parametrize("B,K,every,pitch,candidates,form", CASES)
def test_two_launches_into_a_primed_buffer_equal_single_steps(B, K, every, pitch, candidates, form):
    a, b = _single(B, 2 * K), _single(B, 2 * K)
    out = _registered(b, b.alloc_rollout_buffers(K, obs_every=every, obs_env_pitch=pitch, candidates=candidates))
    assert _flag(b, out["obs"]) == 1
    _is_form(_describe(b, out["obs"], K), form)
    acts = _acts(2 * K, B)
    n_done = 0
    for l in range(2):
        obs, rew, done, info = b.rollout(acts[l * K:(l + 1) * K], out=out, obs_every=every)
        assert obs.data_ptr() == out["obs"].data_ptr() and _flag(b, out["obs"]) == 1
        for k in range(K):
            o, r, d, i = a.step(acts[l * K + k])
            if (k + 1) % every == 0:
                assert torch.equal(o, obs[k // every]), "observations differ at launch %d step %d" % (l, k)
            assert torch.equal(r, rew[k]) and torch.equal(d, done[k])
            assert torch.equal(i["individual_reward"], info["individual_reward"][k])
            n_done += int(d[:, 0].sum())
    assert n_done >= B // 3 - 2                                # those episodes really ended inside the launches
    for x, y in zip(a.world.get_state(), b.world.get_state()):
        assert torch.equal(x, y)
    assert torch.equal(a.world.step_count, b.world.step_count)


@pytest.mark.parametrize("B,K,candidates,form", [(2056, 12, 8, "stream512"), (3080, 8, 1, "stream256"), (2056, 2, 8, "plain16"),
                                                 (40, 5, 8, "small2"), (20, 5, 8, "small2")])
def test_only_whole_lines_inside_the_zero_block_are_left_out(B, K, candidates, form):
    """A registered buffer filled with a sentinel afterwards: what the flagged launch leaves untouched is exactly allowed to
    be whole 128-byte lines (by device address) inside one row's units [N, 2N-1) - and it is at least a third of those bytes
    (the aligned-line rule alone gives 88 of 208 bytes per row = 42 % over the 8-byte phases rows start at)."""
    S = 12345.0
    a, b = _single(B, K), _single(B, K)
    out = _registered(b, b.alloc_rollout_buffers(K, candidates=candidates))
    _is_form(_describe(b, out["obs"], K), form)
    out["obs"].fill_(S)                                        # the registration stays: the launch trusts it
    assert _flag(b, out["obs"]) == 1
    plain = {k: torch.empty_like(v) for k, v in out.items()}
    plain["obs"] = torch.full((K, B, N, D), S, device="cuda")
    assert _flag(a, plain["obs"]) == 0
    acts = _acts(K, B)
    b.rollout(acts, out=out)
    a.rollout(acts, out=plain)
    for k in ("reward", "indiv", "done"):
        assert torch.equal(out[k], plain[k])
    base = out["obs"].data_ptr()
    slot = B * N * D
    i = torch.arange(slot, device="cuda", dtype=torch.int64)
    env_first = (i // (N * D)) * (N * D)                       # first float of the element's env block, in the slot
    unit = (i % D) // 2                                        # 8-byte unit of the element in its row
    in_block = (unit >= N) & (unit < 2 * N - 1)
    survivors = 0
    for s in range(K):
        got, want = out["obs"][s].reshape(-1), plain["obs"][s].reshape(-1)
        diff = got != want
        addr = base + 4 * (s * slot + i)
        g0 = addr - addr % G                                   # the aligned group around the element, by device address
        rel = g0 - (base + 4 * (s * slot + env_first))         # ... relative to its env block
        row, off = rel // (4 * D), rel % (4 * D)
        whole = (rel >= 0) & (row < N) & (off >= 8 * N) & (off + G <= 8 * (2 * N - 1))
        assert bool((in_block | ~diff).all()), "a difference outside the zero block, slot %d" % s
        assert bool((got[diff] == S).all()) and bool((want[diff] == 0).all())
        assert bool((whole | ~diff).all()), "a skipped element outside a whole aligned group of the zero block, slot %d" % s
        survivors += int(diff.sum())
    total = K * B * N * 2 * (N - 1)
    print("survivors: %d of %d zero-block floats = %.3f" % (survivors, total, survivors / total))
    assert 3 * survivors >= total


def test_everything_else_runs_with_the_flag_off():
    from formation_gym import placement
    B, K = 40, 5
    a, b = _single(B, K), _single(B, K)
    acts = _acts(K, B)
    ref = a.rollout(acts, out=False)[0].clone()
    out = _registered(b, b.alloc_rollout_buffers(K))
    snap = b._snapshot()

    def again(o, **kw):
        b._restore(snap)
        return b.rollout(acts, out=o, **kw)[0]

    # a buffer the caller made itself
    own = {k: torch.empty_like(v) for k, v in out.items()}
    assert _flag(b, own["obs"]) == 0 and torch.equal(again(own), ref)
    # 16-bit observations
    h = dict(own, obs=torch.empty((K, B, N, D), dtype=torch.float16, device="cuda"))
    assert _flag(b, h["obs"]) == 0 and torch.equal(again(h, obs_dtype=torch.float16), ref.to(torch.float16))
    # primed=False
    off = b.alloc_rollout_buffers(K, primed=False)
    assert "zero_primed" not in b.placement and _flag(b, off["obs"]) == 0 and torch.equal(again(off), ref)
    # a view that starts mid-slot (four envs in: 16-byte aligned, as the library asks): not flagged - and it puts rows where
    # the buffer's own launches expect zeros, so the registration goes
    big = _registered(b, b.alloc_rollout_buffers(K + 1))
    assert _flag(b, big["obs"]) == 1 and _flag(b, big["obs"][1:]) == 1
    mid = big["obs"].view(-1)[4 * N * D:4 * N * D + K * B * N * D].view(K, B, N, D)
    assert _flag(b, mid) == 0 and _flag(b, big["obs"]) == 0
    assert torch.equal(again(dict(own, obs=mid)), ref)
    assert _flag(b, b.prime_rollout_buffers(big)["obs"]) == 1
    # a world with a non-silent agent: the launch writes the communication block, the registration is dropped
    assert _flag(b, out["obs"]) == 1
    b.world.agents[1].silent = False
    gen = placement.primed_generation()
    assert _flag(b, out["obs"]) == 0
    b.scenario.rollout_batch(b.world, acts, out, auto_reset=True, rng_offset=1)
    torch.cuda.synchronize()
    assert placement.primed_generation() != gen
    b.world.agents[1].silent = True
    assert _flag(b, out["obs"]) == 0                           # silent again, but the buffer is no longer known to hold zeros
    assert _flag(b, b.prime_rollout_buffers(out)["obs"]) == 1
    assert torch.equal(again(out), ref)
