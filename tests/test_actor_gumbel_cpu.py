"""CPU-side tests of the Gumbel-softmax (MADDPG's discrete-action) actor rollout: the draws of tests/actor_gumbel_testlib.py
against hand-computed Philox words, the path rule of `GumbelSoftmaxActor`, the record's binding key, the C ABI of the six new
entries without a device, and the reference at the GPU tests' shapes and seeds: its mutants are told apart, the reference alone
keeps the exempt share of tests/test_gpu_actor_gumbel.py under its cap (1 %), and max |y| < 64 (the sum's rounding of the band).

Expected shares of the mutants (values the GPU tests compare), asserted below:
  actor_stream, blocks_swapped, base_dropped   other, independent Philox blocks: >= 99 % of the draws differ (GPU test 1 compares
                  every draw within gamma <= 8.9e-6), and the exploring indices differ in >= 0.15 of the rows.
  draw4_word3_block0   draw 4 alone is another word: exactly 1 / 5 of the draws (>= 0.199), >= 0.02 of the indices.
  shift8_no_half  u = (c >> 8) 2^-24: one more low bit and no half - u moves by 2^-25 in every draw, and g by du / (u |ln u|),
                  which exceeds gamma only where u |ln u| < ~0.03 (u below ~0.006 or next to 1): >= 1 % of the draws (1.8 %
                  here, 70 to 170 draws per case) and u = 0 gives g = -inf; the indices do not move, so the draws' test alone
                  tells it.
  offset_not_advanced   steps 1 and 2 of the K = 3 launch redraw step 0's: 2 / 3 of the draws (>= 0.66), >= 0.1 of the indices.
  noise_dropped   y = l while exploring: the exploring indices differ wherever the noise changes the argmax, >= 0.15 of rows.
  noise_when_not_exploring   y = l + g while not exploring: the same rows, on the non-exploring launch.
  highest_tie     touches ties only: exactly the tied rows of the standalone inputs (2 of every 64), in both modes of `explore`.
  modes_swapped   every index 1..4 decodes to the opposite sign: exactly the rows with idx != 0, >= 0.4.
  head_rows_agent0   agents 1.. of the per-agent forms get agent 0's head: >= 0.3 of those agents' indices (distinct members).
"""
import copy
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import formation_gym
from formation_gym import (CategoricalActor, GaussianActor, GumbelSoftmaxActor, InputBatchNorm, OUNoiseActor, PerAgentActor,
                           _native, load_scenario)
from formation_gym.actor_rollout import (ACT_ARGMAX, ACT_INDEX, ACT_ONEHOT5, FUSED_N, FusedActor, actor_path, resolve_actor)
from tests import actor_cat_testlib as ct
from tests import actor_gumbel_testlib as gt
from tests import counter_rng as R
from tests.actor_fidelity import ln_actor, rec_actor
from tests.actor_testlib import LIB, ROOT, fake_actor, fake_actors, params as _params

nn = torch.nn
MODES = (ACT_ONEHOT5, ACT_INDEX)


# ---- the draws ----
def _philox_by_hand(c, key, rounds=10):
    """Philox4x32-10 in plain Python integers (Salmon et al. 2011)."""
    c, k = list(c), list(key)
    for _ in range(rounds):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k[0]) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k[1]) & 0xFFFFFFFF, p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_draws_against_hand_computed_philox_words():
    import math
    b, i, N, B = 5, 7, 9, 8
    off = (gt.OFFSET + 2) & R.MASK64                       # step 2 of the launch: the high word is 1
    assert off >> 32 == 1
    key = (gt.SEED & 0xFFFFFFFF, gt.SEED >> 32)
    w0 = _philox_by_hand([b + gt.BASE, i | 0x60000000, off & 0xFFFFFFFF, off >> 32], key)
    w1 = _philox_by_hand([b + gt.BASE, i | 0x60000000 | (1 << 12), off & 0xFFFFFFFF, off >> 32], key)
    words = w0 + [w1[0]]
    want = [-math.log(-math.log((2 * (w >> 9) + 1) / 16777216.0)) for w in words]
    got = gt.launch_gumbels(gt.SEED, gt.BASE, B, N, gt.OFFSET, gt.K)[2, b, i]
    assert np.allclose(got, want, rtol=0, atol=1e-12)
    assert _philox_by_hand([0, 0, 0, 0], (0, 0)) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]   # Random123's vector


def test_every_u_is_strictly_inside_the_unit_interval():
    lo, hi = gt.u_of(np.array([0, 0x1FF], dtype=np.uint64)), gt.u_of(np.array([0xFFFFFFFF, 0xFFFFFE00], dtype=np.uint64))
    assert bool((lo == 2.0 ** -24).all()) and bool((hi == 1.0 - 2.0 ** -24).all())
    for u in (lo, hi):
        assert bool((np.float32(u).astype(np.float64) == u).all())                  # exact in fp32
    assert np.isclose(gt.G_MIN, -2.8115, atol=1e-3) and np.isclose(gt.G_MAX, 16.6355, atol=1e-3)
    assert float(gt.gamma(np.array([gt.G_MIN, gt.G_MAX])).max()) <= 8.9e-6
    g32 = -np.log(-np.log(np.float32([lo[0], hi[0]]), dtype=np.float32), dtype=np.float32)
    assert bool((np.abs(g32.astype(np.float64) - [gt.G_MIN, gt.G_MAX]) <= gt.gamma([gt.G_MIN, gt.G_MAX])).all())


def test_stream_code_is_disjoint_from_every_other_stream():
    mine = {gt.stream_code(i, q) for i in range(1 << 12) for q in (0, 1)}
    assert len(mine) == 2 << 12 and all(c >> 29 == 0b011 for c in mine)
    idx = range(1 << 12)
    for name, fn in R.STREAM_CODES.items():
        others = {fn()} if name == "hd_ivel" else ({fn(i, q) for i in idx for q in range(4)} if name == "comm_noise"
                                                   else {fn(i) for i in idx})
        assert not (mine & others), name
        assert all((c >> 29) in (0b000, 0b001, 0b100, 0b101, 0b110, 0b111) for c in others), name


# ---- the path rule ----
def _mlp(N, H=64, head=5, tanh=False, bn=None):
    mods = [nn.Linear(6 * N, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, head)] + ([nn.Tanh()] if tanh else [])
    if bn is not None:
        mods = [bn(6 * N)] + mods
    return nn.Sequential(*mods).eval()


def test_exported_and_the_four_forms_fuse_in_both_modes():
    assert "GumbelSoftmaxActor" in formation_gym.__all__
    for form in gt.FORMS:
        bn, pa = form in ("bn", "pa_bn"), form in ("pa", "pa_bn")
        for N in FUSED_N:
            for H in ((32, 64) if bn else (32, 64, 128)):
                norm = None if not bn else (nn.BatchNorm1d if pa else InputBatchNorm)
                logits = PerAgentActor([_mlp(N, H, bn=norm) for _ in range(N)]) if pa else _mlp(N, H, bn=norm)
                actor = GumbelSoftmaxActor(logits)
                for mode in MODES:
                    f = resolve_actor(actor, N, continuous=False, action_mode=mode)
                    assert isinstance(f, FusedActor) and f.gumbel is actor and f.cat is None and f.ou is None, (form, N, H)
                    assert f.log_std is None and f.norms is None and f.gru is None
                    assert f.per_agent == pa and (f.in_bn is not None) == bn and len(f.members) == (N if pa else 1)
                    assert f.hidden == H and f.out_tanh is False and tuple(f.members[-1][4].shape) == (5, H)
                    assert len(f.binding_key()) == 7
    a = gt.gumbel_actor("pa_bn", 9, 64)
    assert actor_path(a, 9, continuous=False, action_mode=ACT_ONEHOT5) == "fused"


def test_what_runs_host_paced_and_what_has_no_path():
    N = 9
    good = gt.gumbel_actor("bn", N, 64)
    kw = dict(continuous=False, action_mode=ACT_ONEHOT5)
    assert actor_path(good, N, **kw) == "fused"
    mixed = PerAgentActor([_mlp(N, bn=nn.BatchNorm1d if i % 2 else None) for i in range(N)])
    widths = PerAgentActor([_mlp(N, H=32 if i else 64) for i in range(N)])
    train = _mlp(N, bn=InputBatchNorm).train()
    host = [GumbelSoftmaxActor(ct.cat_actor("ln", N, 64).logits), GumbelSoftmaxActor(ct.cat_actor("gru", N, 32).logits),
            GumbelSoftmaxActor(_mlp(N, head=2)), GumbelSoftmaxActor(_mlp(N, head=4)), GumbelSoftmaxActor(_mlp(N, head=6)),
            GumbelSoftmaxActor(_mlp(N, tanh=True)), GumbelSoftmaxActor(mixed), GumbelSoftmaxActor(widths),
            GumbelSoftmaxActor(_mlp(N, H=128, bn=InputBatchNorm)), GumbelSoftmaxActor(train),
            GumbelSoftmaxActor(PerAgentActor([_mlp(N, H=128, bn=nn.BatchNorm1d) for _ in range(N)])),
            GumbelSoftmaxActor(PerAgentActor([_mlp(N) for _ in range(N - 1)])), GumbelSoftmaxActor(_mlp(N, H=48)),
            gt.gumbel_actor("plain", N, 64, head=4), gt.gumbel_actor("pa", N, 64, tanh=True),
            GumbelSoftmaxActor(lambda o: o[..., :5]), gt.gumbel_actor("plain", N, 64).double()]
    for a in host:
        assert actor_path(a, N, **kw) == "host", a
    assert actor_path(gt.gumbel_actor("plain", 5, 64), 5, **kw) == "host"              # N without a kernel
    for fact in (dict(world_options=True), dict(callback=True), dict(silent=False), dict(fused_scenario=False),
                 dict(fused_gumbel=False)):
        assert actor_path(good, N, **dict(kw, **fact)) == "host", fact
    assert actor_path(gt.gumbel_actor("pa", N, 64), N, per_agent=False, **kw) == "host"
    assert actor_path(good, N, **dict(kw, fused_cat=False, fused_ou=False)) == "fused"  # other members' facts
    # ARGMAX, a continuous env and a bare continuous=False: nothing fuses
    assert resolve_actor(good, N, continuous=False, action_mode=ACT_ARGMAX) is None
    assert resolve_actor(good, N) is None and resolve_actor(good, N, continuous=False) is None


def test_rollout_actor_refuses_a_continuous_env_and_argmax():
    """`MultiAgentEnv.rollout_actor`'s own checks, which come before anything touches a device."""
    from formation_gym import MultiAgentEnv
    actor = GumbelSoftmaxActor(_mlp(3, 32))
    for mode, exc in ((0, ValueError), (_native.FG_ACT_ARGMAX, NotImplementedError)):
        env = types.SimpleNamespace(_action_mode=lambda mode=mode: mode)
        with pytest.raises(exc):
            MultiAgentEnv.rollout_actor(env, 2, actor)
    env = types.SimpleNamespace(_action_mode=lambda: _native.FG_ACT_ONEHOT5)
    with pytest.raises(NotImplementedError):                                         # any other actor in a discrete mode
        MultiAgentEnv.rollout_actor(env, 2, _mlp(3, 32, head=2))


def test_unchanged_answers_of_the_other_members():
    N = 9
    kw = dict(continuous=False, action_mode=ACT_ONEHOT5)
    assert actor_path(CategoricalActor(PerAgentActor([_mlp(N) for _ in range(N)])), N, **kw) == "host"
    assert actor_path(CategoricalActor(_mlp(N, bn=InputBatchNorm)), N, **kw) == "host"
    assert actor_path(CategoricalActor(PerAgentActor([_mlp(N, bn=nn.BatchNorm1d) for _ in range(N)])), N, **kw) == "host"
    assert actor_path(CategoricalActor(_mlp(N)), N, **kw) == "fused"
    others = [_mlp(N, head=2), ln_actor(N, 64, True), rec_actor(N, 32, True), GaussianActor(_mlp(N, head=2)),
              OUNoiseActor(_mlp(N, head=2)), PerAgentActor([_mlp(N, head=2) for _ in range(N)]),
              _mlp(N, head=2, bn=InputBatchNorm), PerAgentActor([_mlp(N, head=2, bn=nn.BatchNorm1d) for _ in range(N)])]
    for a in others:
        f = resolve_actor(a, N)
        assert f is not None and f.gumbel is None and f.cat is None and len(f.binding_key()) == 6      # every existing kind
    assert len(resolve_actor(CategoricalActor(_mlp(N)), N, **kw).binding_key()) == 7
    assert resolve_actor(_mlp(N, head=5), N) is None and resolve_actor(_mlp(N, head=5, bn=InputBatchNorm), N) is None


@pytest.mark.parametrize("name,N,L,M,num_obs,D", [("basic_formation_env", 3, 3, 0, 0, 18),
                                                  ("formation_hd_obs_env", 4, 4, 3, 0, 28)])
def test_landmark_rule_states_no_gumbel_kernel(name, N, L, M, num_obs, D):
    sc = load_scenario(name)
    world = types.SimpleNamespace(agents=[None] * N, landmarks=[None] * (L + M))
    sc.num_agents, sc.num_landmarks, sc.num_obstacles, sc.num_obs, sc.obs_range = N, L, M, num_obs, 0.0
    facts = sc.actor_fused_rule(world)
    assert facts["fused_gumbel"] is False and facts["fused_cat"] is False
    body = nn.Sequential(nn.Linear(D, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 5))
    assert actor_path(GumbelSoftmaxActor(body), N, fused_scenario=True, continuous=False, action_mode=ACT_ONEHOT5, **facts) == "host"


def test_binding_key_equality_and_inequality():
    N = 9
    for form in gt.FORMS:
        a = gt.gumbel_actor(form, N, 32)
        k1 = resolve_actor(a, N, action_mode=ACT_INDEX).binding_key()
        assert k1 == resolve_actor(a, N, action_mode=ACT_INDEX).binding_key()
        assert k1 == resolve_actor(a, N, action_mode=ACT_ONEHOT5).binding_key()       # the mode is the launch's, not the record's
        a.explore = False
        assert k1 == resolve_actor(a, N, action_mode=ACT_INDEX).binding_key()         # read per launch, not baked in
        assert resolve_actor(GumbelSoftmaxActor(a.logits), N, action_mode=ACT_INDEX).binding_key() != k1   # another module
        assert resolve_actor(copy.deepcopy(a), N, action_mode=ACT_INDEX).binding_key() != k1
        head = (a.logits.actors[N - 1] if form in ("pa", "pa_bn") else a.logits)[-1]
        with torch.no_grad():
            head.weight.add_(1.0)
        assert k1 == resolve_actor(a, N, action_mode=ACT_INDEX).binding_key()         # updated in place
        f = resolve_actor(a, N, action_mode=ACT_INDEX)
        assert any(t is head.weight for t in f.tensors()) and any(t is head.bias for t in f.tensors())
        head.weight = nn.Parameter(head.weight.detach().clone())
        assert k1 != resolve_actor(a, N, action_mode=ACT_INDEX).binding_key()         # re-allocated


# ---- the module ----
def test_forward_is_the_one_hot_of_the_argmax():
    N, B = 3, 17
    actor = gt.gumbel_actor("plain", N, 32).double()
    obs = gt.cpu_observations(N, B)
    lg = actor.logits(obs)
    g = torch.as_tensor(gt.gumbels(gt.SEED, gt.BASE, B, N, gt.OFFSET))
    out = actor(obs, g)
    assert out.shape == (B, N, 5) and bool((out.sum(-1) == 1).all())
    assert np.array_equal(out.argmax(-1).numpy(), gt.pick(lg.detach().numpy(), g.numpy(), True)[0])
    torch.manual_seed(0)
    drawn = actor(obs)
    assert drawn.shape == (B, N, 5) and bool((drawn.sum(-1) == 1).all()) and not torch.equal(drawn.argmax(-1), lg.argmax(-1))
    actor.explore = False                                                            # read at every call
    assert torch.equal(actor(obs).argmax(-1), lg.argmax(-1)) and torch.equal(actor(obs, g).argmax(-1), lg.argmax(-1))
    tie = GumbelSoftmaxActor(lambda o: torch.tensor([[1.0, 3.0, 3.0, 0.0, 3.0]]), explore=False)
    assert tie(None).tolist() == [[0.0, 1.0, 0.0, 0.0, 0.0]]                         # ties: the lowest index
    assert "temperature" in GumbelSoftmaxActor.__doc__


# ---- the C ABI without a device ----
ENTRIES = ("fg_rollout_hd_actor_gumbel", "fg_rollout_hd_actor_gumbel_per_agent", "fg_describe_actor_gumbel_launch",
           "fg_describe_actor_gumbel_per_agent_launch", "fg_actor_gumbel", "fg_actor_gumbel_pick")
KERNEL = {"plain": "gumbel_actor_kernel", "pa": "pa_gumbel_actor_kernel", "bn": "bn_gumbel_actor_kernel",
          "pa_bn": "pa_bn_gumbel_actor_kernel"}


def _bn(**kw):
    d = dict(mean=4096, var=4096, gamma=4096, beta=4096, eps=1e-5)
    d.update(kw)
    return _native.FgActorInBn(**d)


def _call(lib, dry, form="plain", N=9, K=20, B=128, H=64, tanh=0, mode=ACT_ONEHOT5, explore=1, idx=4096, actor="fake", bn="fake"):
    """(status, fg_last_error(), text) of the form's Gumbel entry (its describe twin when `dry`) on stand-in pointers."""
    pa, has_bn = form in ("pa", "pa_bn"), form in ("bn", "pa_bn")
    fa = (fake_actors(N, H, tanh) if pa else fake_actor(H, tanh)) if actor == "fake" else actor
    fb = None
    if has_bn:
        fb = ((_native.FgActorInBn * N)(*[_bn() for _ in range(N)]) if pa else _bn()) if bn == "fake" else bn
    sfx = "_per_agent" if pa else ""
    text = ""
    if dry:
        buf = ctypes.create_string_buffer(512)
        rc = getattr(lib, "fg_describe_actor_gumbel%s_launch" % sfx)(_params(), fa, fb, mode, explore, B, N, K, 1, buf, 512)
        text = buf.value.decode()
    else:
        rc = getattr(lib, "fg_rollout_hd_actor_gumbel" + sfx)(_params(), fa, fb, mode, explore, B, N, K,
                                                              *([ctypes.c_void_p(4096)] * 12), idx, 1, None)
    return rc, lib.fg_last_error().decode(), text


def test_symbols_exported_declared_and_bound():
    lib = ctypes.CDLL(LIB)
    header = open(os.path.join(ROOT, "include", "formation_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _native.SIGNATURES and ("int %s(" % name) in header and name in doc, name
    assert _native.load().fg_abi_version() == 8                                    # an additive change


def test_status_codes_without_a_device():
    lib = _native.load()
    for dry in (False, True):
        for form in gt.FORMS:
            pa, has_bn = form in ("pa", "pa_bn"), form in ("bn", "pa_bn")
            who = "fg_rollout_hd_actor_gumbel" + ("_per_agent" if pa else "")
            bad = lambda **kw: _call(lib, dry, form, **kw)[:2]
            assert bad(tanh=1) == (-1, who + ": out_tanh must be 0: the head's outputs are logits")
            for mode in (0, ACT_ARGMAX, 4, -1):
                assert bad(mode=mode) == (-1, who + ": act_mode must be FG_ACT_ONEHOT5 or FG_ACT_INDEX"), mode
            # the inner entry's checks, in their order and with their texts
            assert bad(H=48) == (-1, "fg_rollout_hd_actor: hidden must be 32, 64 or 128")
            assert bad(N=5)[0] == -2 and bad(N=81)[0] == -2 and bad(K=0)[0] == -1 and bad(actor=None)[0] == -1
            assert bad(H=48, tanh=1, mode=0)[1] == "fg_rollout_hd_actor: hidden must be 32, 64 or 128"   # the actor first
            if has_bn:
                assert bad(H=128)[0] == -1 and "hidden must be 32 or 64 with an input BatchNorm" in bad(H=128)[1]
                assert bad(H=128, tanh=1)[1].endswith("hidden must be 32 or 64 with an input BatchNorm")  # then the BatchNorm
            else:
                assert _call(lib, True, form, H=128)[0] == 0
    for form in gt.FORMS:                                  # the launch's own buffer
        who = "fg_rollout_hd_actor_gumbel" + ("_per_agent" if form in ("pa", "pa_bn") else "")
        bad = lambda **kw: _call(lib, False, form, **kw)[:2]
        assert bad(idx=None) == (-1, who + ": idx_seq is NULL")
        assert bad(idx=4098) == (-3, who + ": idx_seq must be 4-byte aligned")
        assert bad(B=0)[0] == 0 and bad(B=0, idx=None)[0] == 0                       # an empty batch is a no-op ...
        assert bad(B=0, tanh=1)[0] == -1 and bad(B=-1)[0] == -1                      # ... after the checks
        assert _call(lib, True, form, B=0)[:2] == (-1, "fg_describe_actor_launch: B > 0 required")
    assert lib.fg_describe_actor_gumbel_launch(_params(), fake_actor(64, 0), None, ACT_INDEX, 1, 128, 9, 20, 1, None, 0) == -1
    bn1 = _bn(eps=0.0)
    assert _call(lib, True, "bn", bn=bn1) == (-1, "fg_rollout_hd_actor_gumbel: in_bn eps must be positive and finite", "")


def test_describe_names_exactly_the_eighty_instantiations():
    lib = _native.load()
    names = set()
    for form in gt.FORMS:
        for N in FUSED_N:
            for H in ((32, 64) if form in ("bn", "pa_bn") else (32, 64, 128)):
                texts = set()
                for mode in MODES:
                    for explore in (0, 1):
                        rc, err, text = _call(lib, True, form, N=N, H=H, B=4096, mode=mode, explore=explore)
                        assert rc == 0, (form, N, H, err)
                        texts.add(text)
                assert len(texts) == 1                                              # the mode and the flag pick no kernel
                text = texts.pop()
                G = 4 if N <= 4 else 8 if N <= 8 else 16 if N <= 16 else 32
                E = 256 // G
                assert text.startswith("%s<%d,%d> grid %d block 256 envs/wg %d lds " % (KERNEL[form], N, H, -(-4096 // E), E)), text
                lds = int(text.split("lds ")[1].split(";")[0])
                assert 0 < lds <= 160 * 1024, (form, N, H, lds)
                names.add(text.split(" grid")[0])
    assert len(names) == 24 + 24 + 16 + 16


def test_helpers_reject_bad_arguments_without_a_device():
    lib = _native.load()
    gum, pk = lib.fg_actor_gumbel, lib.fg_actor_gumbel_pick
    p = _params()
    assert gum(p, 0, 3, 4096, None) == 0 and gum(p, -1, 3, 4096, None) == -1 and gum(p, 4, 0, 4096, None) == -1
    assert gum(p, 4, 3, None, None) == -1 and gum(p, 4, 3, 4098, None) == -3 and gum(None, 4, 3, 4096, None) == -1
    assert gum(p, 4, (1 << 12) + 1, 4096, None) == -1                                # the stream's codes: agents below 2^12
    ok = (4096, 4096, 4096, 4096, None)
    assert pk(ACT_INDEX, 1, 0, *ok) == 0 and pk(ACT_ONEHOT5, 0, 0, None, None, None, None, None) == 0
    assert pk(ACT_ARGMAX, 1, 8, *ok) == -1 and pk(0, 1, 8, *ok) == -1 and pk(ACT_INDEX, 1, -1, *ok) == -1
    assert pk(ACT_INDEX, 1, 8, None, 4096, 4096, 4096, None) == -1
    assert pk(ACT_INDEX, 1, 8, 4096, None, 4096, 4096, None) == -1                   # exploring needs g
    assert pk(ACT_INDEX, 1, 8, 4096, 4096, None, 4096, None) == -1
    assert pk(ACT_INDEX, 1, 8, 4098, 4096, 4096, 4096, None) == -3
    assert pk(ACT_INDEX, 1, 8, 4096, 4096, 4096, 4100, None) == -3                   # act: 8-byte


# ---- the reference at the GPU tests' inputs: mutants, coverage, the exempt share ----
_SHAPES = list(dict.fromkeys(c[:4] for c in gt.CASES))              # every (form, N, B, H) of the GPU tests, once


def _reference_case(form, N, B, H, mutant=None):
    """(logits [K, B, N, 5], beta [K, B, N]) of the fp64 actor on K draws of oracle observations: the distribution of the GPU
    tests' rows (their steps act on observations of the same envs a step later)."""
    actor = gt.double(gt.gumbel_actor(form, N, H))
    out = [gt.logits64(actor, form, gt.cpu_observations(N, B, seed=1 + k), mutant) for k in range(gt.K)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


@pytest.mark.parametrize("form,N,B,H", _SHAPES)
def test_mutants_differ_and_the_reference_stays_under_the_cap(form, N, B, H):
    lg, beta = _reference_case(form, N, B, H)
    g = gt.launch_gumbels(gt.SEED, gt.BASE, B, N, gt.OFFSET, gt.K)
    assert np.isfinite(g).all() and g.min() >= gt.G_MIN and g.max() <= gt.G_MAX
    assert float(np.abs(lg + g).max()) < gt.Y_MAX and float(np.abs(lg).max()) < gt.Y_MAX    # the sum's rounding: 2^-19
    idx, margin = gt.pick(lg, g, True)
    idx0, margin0 = gt.pick(lg, None, False)
    assert set(np.unique(idx).tolist()) == {0, 1, 2, 3, 4}
    # the exempt share of the fp64 reference alone, at the bands the GPU test uses: at most 1 % of the rows
    share, share0 = float(gt.exempt(margin, beta, g, True).mean()), float(gt.exempt(margin0, beta, None, False).mean())
    assert share <= gt.EXEMPT_CAP and share0 <= gt.EXEMPT_CAP, (share, share0)
    # the torch fp32 actor against the fp64 one: rows outside the band pick the same index
    a32 = gt.gumbel_actor(form, N, H)
    for k in range(gt.K):
        with torch.no_grad():
            l32 = a32.logits(gt.cpu_observations(N, B, seed=1 + k).float()).double().numpy()
        for explore, want, mg in ((True, idx, margin), (False, idx0, margin0)):
            keep = ~gt.exempt(mg[k], beta[k], g[k], explore)
            assert np.array_equal(gt.pick(l32, g[k], explore)[0][keep], want[k][keep])
    noise_moves = float((idx != idx0).mean())
    assert noise_moves >= 0.15, noise_moves
    for m in ("actor_stream", "blocks_swapped", "base_dropped", "draw4_word3_block0", "shift8_no_half", "offset_not_advanced"):
        gm = gt.launch_gumbels(gt.SEED, gt.BASE, B, N, gt.OFFSET, gt.K, m)
        with np.errstate(invalid="ignore"):
            drew = float((~(np.abs(gm - g) <= gt.gamma(g))).mean())
        moved = float((gt.pick(lg, gm, True)[0] != idx).mean())
        low = {"draw4_word3_block0": (0.199, 0.02), "shift8_no_half": (0.01, 0.0), "offset_not_advanced": (0.66, 0.1)}.get(m, (0.99, 0.15))
        assert drew >= low[0] and moved >= low[1], (m, drew, moved)
    assert float((gt.pick(lg, g, True, "noise_dropped")[0] != idx).mean()) == noise_moves
    assert float((gt.pick(lg, g, False, "noise_when_not_exploring")[0] != idx0).mean()) == noise_moves
    assert np.array_equal(gt.pick(lg, g, True, "highest_tie")[0], idx)              # ties only: below
    for mode in (gt.ONEHOT5, gt.INDEX):
        act, swapped = gt.decode(mode, idx), gt.decode(mode, idx, "modes_swapped")
        assert float((act != swapped).any(-1).mean()) == float((idx != 0).mean()) >= 0.4
    if form in ("pa", "pa_bn"):
        lgm = _reference_case(form, N, B, H, "head_rows_agent0")[0]
        assert np.array_equal(lgm[:, :, 0], lg[:, :, 0])
        for explore, want in ((True, idx), (False, idx0)):
            moved = float((gt.pick(lgm, g, explore)[0] != want)[:, :, 1:].mean())
            assert moved >= 0.3, (explore, moved)


def test_tie_mutant_and_edge_rows_of_the_standalone_inputs():
    lg, g = gt.standalone_inputs()
    l64, g64 = lg.astype(np.float64), g.astype(np.float64)
    rows = np.arange(len(lg))
    tied = (rows % 64 == 2) | (rows % 64 == 3)
    for explore in (True, False):
        idx, margin = gt.pick(l64, g64, explore)
        im = gt.pick(l64, g64, explore, "highest_tie")[0]
        assert np.array_equal(idx != im, tied)                                     # exactly the tied rows
        assert bool((margin[tied] == 0).all()) and bool((idx[rows % 64 == 2] == 1).all()) and bool((idx[rows % 64 == 3] == 0).all())
        assert bool((idx[rows % 64 == 1] == 3).all()) and bool((idx[rows % 64 == 4] != 2).all())      # +/-100
        assert set(np.unique(idx).tolist()) == {0, 1, 2, 3, 4}
        band = 2.0 * gt.gamma(g64).max(-1) + gt.SUM_ROUNDING if explore else 0.0
        assert float(((margin <= band) & ~tied).mean()) < 0.01
    assert float(g.max()) == np.float32(gt.G_MAX) and float(g.min()) == np.float32(gt.G_MIN)             # the extreme draws
