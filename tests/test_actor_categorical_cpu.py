"""CPU-side tests of the categorical (discrete-action) actor rollout: the path rule of `CategoricalActor`, the module against
torch.distributions.Categorical, the C ABI of `fg_rollout_hd_actor_cat`, `fg_describe_actor_cat_launch`, `fg_actor_uniform` and
`fg_actor_categorical` without a device, and the reference of tests/actor_cat_testlib.py: its mutants are told apart at the GPU
tests' shapes and seeds, all five indices occur, and the reference alone keeps the exempt share of
tests/test_gpu_actor_categorical.py under its cap.

Expected shares of the mutants (values the GPU tests compare; `_mutant_shares`), each derived from the reference's own
probabilities p_j of the rows and asserted at 0.8 of the expectation (a few hundred to two thousand rows per case):
  word0, word3, base_dropped   another, independent uniform draw: the draw itself, which GPU test 1 compares bit for bit,
                  differs in >= 99 % of the values (2^-24 collisions); two independent draws pick different indices with
                  probability 1 - sum_j p_j^2, whose mean over the rows is the expected share of the indices (0.2 to 0.7 here).
  offset_not_advanced   the same for steps 1 and 2 of the K = 3 launch, step 0 unchanged: 2 / 3 of both shares.
  t_is_u          t = u instead of u s, s in [1, 5]: the same index only where u and u / s fall into one CDF cell; no closed
                  form is used, the share must be at least 0.1 (it is 0.2 to 0.7).
  descending_cumsum   the CDF of the reversed classes: the same index only where u lands in a cell common to both orders;
                  likewise at least 0.1 (0.4 to 0.9).
  modes_swapped   the two sign conventions exchanged: every index 1..4 decodes to the opposite sign - exactly the share of rows
                  with idx != 0, 1 - mean p_0, at least 0.5 here; the indices themselves do not change.
  axes_swapped    x and y exchanged: likewise every index 1..4.
  greedy_highest_tie  touches ties only: exactly the rows of the standalone inputs built with tied maxima (3 of every 64 rows),
                  share 1 there, 0 elsewhere.
  logp_of_greedy  the log-prob of the mode while sampling: differs wherever the sampled index is not the mode, expected share
                  1 - mean max_j p_j (0.15 to 0.5 here).
"""
import copy
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import formation_gym
from formation_gym import CategoricalActor, GaussianActor, InputBatchNorm, OUNoiseActor, PerAgentActor, _native, load_scenario
from formation_gym.actor_rollout import (ACT_ARGMAX, ACT_INDEX, ACT_ONEHOT5, FUSED_N, FusedActor, actor_path, recurrent_mean,
                                         resolve_actor)
from tests import actor_cat_testlib as ct
from tests.actor_fidelity import ln_actor, rec_actor
from tests.actor_testlib import LIB, ROOT, fake_actor, params as _params

nn = torch.nn
MODES = (ACT_ONEHOT5, ACT_INDEX)


def _mlp(N, H=64, head=2, tanh=False):
    mods = [nn.Linear(6 * N, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, head)] + ([nn.Tanh()] if tanh else [])
    return nn.Sequential(*mods)


# ---- the path rule ----
def test_exported_and_the_three_forms_fuse_in_both_modes():
    assert "CategoricalActor" in formation_gym.__all__ and (ACT_ONEHOT5, ACT_INDEX, ACT_ARGMAX) == \
        (_native.FG_ACT_ONEHOT5, _native.FG_ACT_INDEX, _native.FG_ACT_ARGMAX)
    N = 9
    for fam in ("plain", "ln", "gru"):
        for H in (32, 64):
            actor = ct.cat_actor(fam, N, H)
            for mode in MODES:
                f = resolve_actor(actor, N, continuous=False, action_mode=mode)
                assert isinstance(f, FusedActor) and f.cat is actor and f.log_std is None and f.ou is None and not f.per_agent
                assert (f.norms is not None) == (fam != "plain") and (f.gru is not None) == (fam == "gru")
                assert f.hidden == H and f.out_tanh is False and tuple(f.members[0][4].shape) == (5, H)
                assert actor_path(actor, N, continuous=False, action_mode=mode) == "fused"
            assert (recurrent_mean(actor) is not None) == (fam == "gru")
    assert actor_path(ct.cat_actor("plain", 3, 128), 3, action_mode=ACT_INDEX) == "fused"
    for n in FUSED_N:
        assert actor_path(ct.cat_actor("ln", n, 32), n, action_mode=ACT_ONEHOT5) == "fused"


def test_what_runs_host_paced_and_what_has_no_path():
    N = 9
    good = ct.cat_actor("ln", N, 64)
    kw = dict(continuous=False, action_mode=ACT_ONEHOT5)
    assert actor_path(good, N, **kw) == "fused"
    host = [CategoricalActor(_mlp(N, head=4)), CategoricalActor(_mlp(N, head=2)), CategoricalActor(_mlp(N, head=6)),
            CategoricalActor(_mlp(N, head=5, tanh=True)),
            CategoricalActor(PerAgentActor([_mlp(N, head=5) for _ in range(N)])),
            CategoricalActor(nn.Sequential(InputBatchNorm(6 * N), *_mlp(N, head=5)).eval()),
            ct.cat_actor("ln", N, 128), ct.cat_actor("gru", N, 128), ct.cat_actor("plain", N, 48),
            CategoricalActor(lambda o: o[..., :5]), ct.cat_actor("plain", N, 64).double()]
    rec_tanh = ct.cat_actor("gru", N, 32)
    rec_tanh.logits.head = nn.Sequential(rec_tanh.logits.head, nn.Tanh())
    host.append(rec_tanh)
    for a in host:
        assert actor_path(a, N, **kw) == "host", a
    assert actor_path(ct.cat_actor("plain", 5, 64), 5, **kw) == "host"                 # N without a kernel
    for fact in (dict(world_options=True), dict(callback=True), dict(silent=False), dict(fused_scenario=False),
                 dict(fused_cat=False)):
        assert actor_path(good, N, **dict(kw, **fact)) == "host", fact
    # ARGMAX, a continuous env and a bare continuous=False: nothing fuses
    assert resolve_actor(good, N, continuous=False, action_mode=ACT_ARGMAX) is None
    assert resolve_actor(good, N) is None and resolve_actor(good, N, continuous=False) is None
    # every other actor in a discrete mode: None, as before
    others = [_mlp(N), ln_actor(N, 64, True), rec_actor(N, 32, True), GaussianActor(_mlp(N)), OUNoiseActor(_mlp(N)),
              PerAgentActor([_mlp(N) for _ in range(N)])]
    for a in others:
        assert resolve_actor(a, N) is not None
        assert resolve_actor(a, N).cat is None and len(resolve_actor(a, N).binding_key()) == 6     # an unchanged answer
        for mode in (ACT_ONEHOT5, ACT_INDEX, ACT_ARGMAX):
            assert resolve_actor(a, N, continuous=False, action_mode=mode) is None
            assert resolve_actor(a, N, action_mode=mode) is None
        assert resolve_actor(a, N, continuous=False) is None
    # a five-output head without the member stays what it was: no two-output kernel takes it
    assert resolve_actor(_mlp(N, head=5), N) is None


@pytest.mark.parametrize("name,N,L,M,num_obs,D", [("basic_formation_env", 3, 3, 0, 0, 18),
                                                  ("formation_hd_obs_env", 4, 4, 3, 0, 28)])
def test_landmark_rule_states_no_categorical_kernel(name, N, L, M, num_obs, D):
    sc = load_scenario(name)
    world = types.SimpleNamespace(agents=[None] * N, landmarks=[None] * (L + M))
    sc.num_agents, sc.num_landmarks, sc.num_obstacles, sc.num_obs, sc.obs_range = N, L, M, num_obs, 0.0
    facts = sc.actor_fused_rule(world)
    assert facts["fused_cat"] is False
    body = nn.Sequential(nn.Linear(D, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 5))
    assert actor_path(CategoricalActor(body), N, fused_scenario=True, continuous=False, action_mode=ACT_INDEX, **facts) == "host"


def test_binding_key_equality_and_inequality():
    N = 9
    a = ct.cat_actor("gru", N, 32)
    k1 = resolve_actor(a, N, action_mode=ACT_INDEX).binding_key()
    assert k1 == resolve_actor(a, N, action_mode=ACT_INDEX).binding_key()
    assert k1 == resolve_actor(a, N, action_mode=ACT_ONEHOT5).binding_key()           # the mode is the launch's, not the record's
    a.deterministic = True
    assert k1 == resolve_actor(a, N, action_mode=ACT_INDEX).binding_key()             # read per launch, not baked in
    twin = CategoricalActor(a.logits)
    assert resolve_actor(twin, N, action_mode=ACT_INDEX).binding_key() != k1          # another module: another flag to read
    b = copy.deepcopy(a)
    assert resolve_actor(b, N, action_mode=ACT_INDEX).binding_key() != k1
    with torch.no_grad():
        a.logits.head.weight.add_(1.0)
    assert k1 == resolve_actor(a, N, action_mode=ACT_INDEX).binding_key()             # updated in place
    a.logits.head.weight = nn.Parameter(a.logits.head.weight.detach().clone())
    assert k1 != resolve_actor(a, N, action_mode=ACT_INDEX).binding_key()             # re-allocated
    f = resolve_actor(a, N, action_mode=ACT_INDEX)
    assert any(t is a.logits.head.weight for t in f.tensors()) and any(t is a.logits.head.bias for t in f.tensors())


# ---- the module ----
@pytest.mark.parametrize("fam", ["plain", "ln", "gru"])
def test_log_prob_entropy_distribution_against_torch(fam):
    N, B = 3, 17
    actor = ct.cat_actor(fam, N, 32).double()
    obs = ct.cpu_observations(N, B)
    h = torch.rand(B, N, 32, dtype=torch.float64) - 0.5 if fam == "gru" else None
    lg = actor.logits(obs, h)[0] if fam == "gru" else actor.logits(obs)
    want = torch.distributions.Categorical(logits=lg)
    idx = torch.randint(0, 5, (B, N), generator=torch.Generator().manual_seed(1))
    args = (h,) if fam == "gru" else ()
    assert torch.allclose(actor.log_prob(obs, idx, *args), want.log_prob(idx), atol=1e-12)
    assert torch.allclose(actor.log_prob(obs, idx.to(torch.int32), *args), want.log_prob(idx), atol=1e-12)
    assert torch.allclose(actor.entropy(obs, *args), want.entropy(), atol=1e-12)
    assert torch.allclose(actor.distribution(obs, *args).probs, want.probs, atol=1e-12)
    # differentiable in the parameters
    (actor.log_prob(obs, idx, *args).sum() + actor.entropy(obs, *args).sum()).backward()
    head = actor.logits.head if fam == "gru" else actor.logits[-1]
    assert head.weight.grad is not None and float(head.weight.grad.abs().max()) > 0
    # forward: samples with torch; `deterministic` is read at every call
    torch.manual_seed(0)
    out = actor(obs, *args)
    s = out[0] if fam == "gru" else out
    assert s.shape == (B, N) and s.dtype == torch.int64 and int(s.min()) >= 0 and int(s.max()) <= 4
    actor.deterministic = True
    out = actor(obs, *args)
    assert torch.equal(out[0] if fam == "gru" else out, lg.argmax(-1))
    if fam == "gru":
        assert torch.equal(out[1], actor.logits(obs, h)[1])


def test_reference_against_torch_log_softmax():
    rng = np.random.RandomState(0)
    lg = rng.standard_normal((500, 5)) * 3
    u = rng.rand(500)
    idx, logp, margin = ct.pick(lg, u)
    lsm = torch.log_softmax(torch.as_tensor(lg), -1).numpy()
    assert np.allclose(logp, np.take_along_axis(lsm, idx[:, None], 1)[:, 0], atol=1e-12)
    cdf = np.cumsum(np.exp(lsm), -1)
    clear = margin > 1e-9                                  # torch's CDF rounds differently right at a boundary
    assert bool(clear.all()) and np.array_equal(idx[clear], np.minimum((u[:, None] >= cdf).sum(-1), 4)[clear])
    g, glogp, gap = ct.pick(lg, greedy=True)
    assert np.array_equal(g, lg.argmax(-1)) and np.allclose(glogp, lsm.max(-1), atol=1e-12) and bool((gap > 0).all())
    assert ct.decode(ct.ONEHOT5, np.arange(5)).tolist() == [[0, 0], [1, 0], [-1, 0], [0, 1], [0, -1]]
    assert ct.decode(ct.INDEX, np.arange(5)).tolist() == [[0, 0], [-1, 0], [1, 0], [0, -1], [0, 1]]
    onehot = np.eye(5)
    assert np.array_equal(ct.decode(ct.ONEHOT5, np.arange(5)), np.stack([onehot[:, 1] - onehot[:, 2], onehot[:, 3] - onehot[:, 4]], -1))


# ---- the C ABI without a device ----
ENTRIES = ("fg_rollout_hd_actor_cat", "fg_describe_actor_cat_launch", "fg_actor_uniform", "fg_actor_categorical")
WHO = "fg_rollout_hd_actor_cat"


def _norm(**kw):
    d = dict(in_gamma=4096, in_beta=4096, h1_gamma=4096, h1_beta=4096, h2_gamma=4096, h2_beta=4096, in_eps=1e-5, h1_eps=1e-5,
             h2_eps=1e-5, in_norm=1)
    d.update(kw)
    return _native.FgActorNorm(**d)


def _gru(**kw):
    d = dict(w_ih=4096, w_hh=4096, b_ih=4096, b_hh=4096, norm_gamma=4096, norm_beta=4096, norm_eps=1e-5)
    d.update(kw)
    return _native.FgActorGru(**d)


def _call(lib, dry, fam="plain", N=9, K=20, B=128, H=64, tanh=0, mode=ACT_ONEHOT5, greedy=0, idx=4096, logp=4096, state=4096,
          states=None, every=1, norm="fake", gru="fake", actor="fake"):
    """(status, fg_last_error(), text) of fg_rollout_hd_actor_cat (its describe twin when `dry`) on stand-in pointers."""
    fa = fake_actor(H, tanh) if actor == "fake" else actor
    fn = None if fam == "plain" else (_norm() if norm == "fake" else norm)
    fg = None if fam != "gru" else (_gru() if gru == "fake" else gru)
    text = ""
    if dry:
        buf = ctypes.create_string_buffer(512)
        rc = lib.fg_describe_actor_cat_launch(_params(), fa, fn, fg, mode, greedy, B, N, K, 1, buf, 512)
        text = buf.value.decode()
    else:
        rc = lib.fg_rollout_hd_actor_cat(_params(), fa, fn, fg, mode, greedy, B, N, K, *([ctypes.c_void_p(4096)] * 12), idx, logp,
                                         state, states, every, 1, None)
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
        for fam in ("plain", "ln", "gru"):
            bad = lambda **kw: _call(lib, dry, fam, **kw)[:2]
            assert bad(tanh=1) == (-1, WHO + ": out_tanh must be 0: the head's outputs are logits")
            for mode in (0, ACT_ARGMAX, 4, -1):
                assert bad(mode=mode) == (-1, WHO + ": act_mode must be FG_ACT_ONEHOT5 or FG_ACT_INDEX"), mode
            # the inherited checks, in their order and with their texts
            assert bad(H=48) == (-1, "fg_rollout_hd_actor: hidden must be 32, 64 or 128")
            assert bad(N=5)[0] == -2 and bad(N=81)[0] == -2 and bad(K=0)[0] == -1 and bad(actor=None)[0] == -1
            if fam != "plain":
                assert bad(H=128) == (-1, WHO + ": hidden must be 32 or 64 with LayerNorms")
                assert bad(norm=_norm(h1_eps=0.0)) == (-1, WHO + ": h1_eps must be positive and finite")
                assert bad(norm=_norm(h2_gamma=4098))[0] == -1
            if fam == "gru":
                assert bad(gru=_gru(w_hh=None)) == (-1, WHO + ": w_hh is NULL")
                assert bad(gru=_gru(norm_eps=float("nan"))) == (-1, WHO + ": norm_eps must be positive and finite")
                assert bad(gru=_gru(b_ih=4098)) == (-3, WHO + ": b_ih must be 4-byte aligned")
    # gru without norm
    buf = ctypes.create_string_buffer(512)
    assert lib.fg_describe_actor_cat_launch(_params(), fake_actor(64, 0), None, _gru(), ACT_INDEX, 0, 128, 9, 20, 1, buf, 512) == -1
    assert lib.fg_last_error().decode() == WHO + ": norm is NULL"
    # the launch's own buffers
    for fam in ("plain", "ln", "gru"):
        bad = lambda **kw: _call(lib, False, fam, **kw)[:2]
        assert bad(idx=None) == (-1, WHO + ": idx_seq is NULL")
        assert bad(idx=4098) == (-3, WHO + ": idx_seq and logp_seq must be 4-byte aligned")
        assert bad(logp=4097) == (-3, WHO + ": idx_seq and logp_seq must be 4-byte aligned")
        assert bad(B=0)[0] == 0 and bad(B=0, idx=None, logp=None)[0] == 0          # an empty batch is a no-op ...
        assert bad(B=0, tanh=1)[0] == -1 and bad(B=-1)[0] == -1                    # ... after the checks
    bad = lambda **kw: _call(lib, False, "gru", **kw)[:2]
    assert bad(state=None) == (-1, WHO + ": rnn_state is NULL")
    assert bad(state=4104)[0] == -3
    assert bad(states=4096, every=0)[0] == -1 and bad(states=4104, every=2)[0] == -3
    assert _call(lib, True, B=0)[:2] == (-1, "fg_describe_actor_launch: B > 0 required")
    assert lib.fg_describe_actor_cat_launch(_params(), fake_actor(64, 0), None, None, ACT_INDEX, 0, 128, 9, 20, 1, None, 0) == -1


def test_describe_names_one_instantiation_per_shape_within_the_lds_budget():
    lib = _native.load()
    names = set()
    kernel = {"plain": "cat_actor_kernel", "ln": "ln_cat_actor_kernel", "gru": "gru_cat_actor_kernel"}
    for fam in ("plain", "ln", "gru"):
        for N in FUSED_N:
            for H in ((32, 64, 128) if fam == "plain" else (32, 64)):
                texts = set()
                for mode in MODES:
                    for greedy in (0, 1):
                        rc, err, text = _call(lib, True, fam, N=N, H=H, B=4096, mode=mode, greedy=greedy)
                        assert rc == 0, (fam, N, H, err)
                        texts.add(text)
                assert len(texts) == 1                                              # the mode and the flag pick no kernel
                text = texts.pop()
                G = 4 if N <= 4 else 8 if N <= 8 else 16 if N <= 16 else 32
                E = 256 // G
                assert text.startswith("%s<%d,%d> grid %d block 256 envs/wg %d lds " % (kernel[fam], N, H, -(-4096 // E), E)), text
                lds = int(text.split("lds ")[1].split(";")[0])
                assert 0 < lds <= 160 * 1024, (fam, N, H, lds)
                names.add(text.split(" grid")[0])
    assert len(names) == 8 * 3 + 8 * 2 + 8 * 2


def test_helpers_reject_bad_arguments_without_a_device():
    lib = _native.load()
    uni, cat = lib.fg_actor_uniform, lib.fg_actor_categorical
    p = _params()
    assert uni(p, 0, 3, 4096, None) == 0 and uni(p, -1, 3, 4096, None) == -1 and uni(p, 4, 0, 4096, None) == -1
    assert uni(p, 4, 3, None, None) == -1 and uni(p, 4, 3, 4098, None) == -3 and uni(None, 4, 3, 4096, None) == -1
    ok = (4096, 4096, 4096, 4096, 4096, None)
    assert cat(ACT_INDEX, 0, 0, *ok) == 0 and cat(ACT_ONEHOT5, 1, 0, None, None, None, None, None, None) == 0
    assert cat(ACT_ARGMAX, 0, 8, *ok) == -1 and cat(0, 0, 8, *ok) == -1 and cat(ACT_INDEX, 0, -1, *ok) == -1
    assert cat(ACT_INDEX, 0, 8, None, 4096, 4096, 4096, 4096, None) == -1
    assert cat(ACT_INDEX, 0, 8, 4096, None, 4096, 4096, 4096, None) == -1          # sampling needs u
    assert cat(ACT_INDEX, 0, 8, 4096, 4096, None, 4096, 4096, None) == -1
    assert cat(ACT_INDEX, 0, 8, 4098, 4096, 4096, 4096, 4096, None) == -3
    assert cat(ACT_INDEX, 0, 8, 4096, 4096, 4096, 4100, 4096, None) == -3          # act: 8-byte


# ---- the reference at the GPU tests' inputs: mutants, coverage, the exempt share ----
def _reference_case(fam, N, B, H):
    """(logits [K, B, N, 5], beta [K, B, N]) of the fp64 actor on K draws of oracle observations: the distribution of the GPU
    tests' rows (their steps act on observations of the same envs a step later)."""
    actor = ct.cat_actor(fam, N, H, seed=ct.case_seed(fam, N, B, H)).double()
    lgs, betas = [], []
    for k in range(ct.K):
        obs = ct.cpu_observations(N, B, seed=1 + k)
        h = (torch.rand(B, N, H, dtype=torch.float64, generator=torch.Generator().manual_seed(k)) - 0.5) if fam == "gru" else None
        lg, beta = ct.logits64(actor, fam, obs, h)[:2]
        lgs.append(lg); betas.append(beta)
    return np.stack(lgs), np.stack(betas)


def _mutant_shares(lg, N, B, mode):
    """{mutant: share of differing values} of what the GPU tests compare for one case: the draws, the indices, the decoded
    actions and the log-probs of a sampled launch."""
    u = ct.launch_uniforms(ct.SEED, ct.BASE, B, N, ct.OFFSET, ct.K)
    idx, logp, _ = ct.pick(lg, u)
    act = ct.decode(mode, idx)
    out = {}
    for m in ct.MUTANTS:
        um = ct.launch_uniforms(ct.SEED, ct.BASE, B, N, ct.OFFSET, ct.K, m)
        im, lm, _ = ct.pick(lg, um, mutant=m)
        am = ct.decode(mode, im, m)
        out[m] = dict(u=float((um != u).mean()), idx=float((im != idx).mean()), act=float((am != act).any(-1).mean()),
                      logp=float((np.abs(lm - logp) > 1e-3).mean()), moved=float((idx != 0).mean()))
    return out


@pytest.mark.parametrize("fam,N,B,H", ct.CASES)
def test_mutants_differ_indices_cover_and_the_reference_stays_under_the_cap(fam, N, B, H):
    lg, beta = _reference_case(fam, N, B, H)
    pmax = np.exp(lg - lg.max(-1, keepdims=True))
    pmax = (pmax / pmax.sum(-1, keepdims=True)).max(-1)
    assert pmax.min() < 0.4 and pmax.max() > 0.9, (pmax.min(), pmax.max())     # near-uniform to nearly decided rows
    u = ct.launch_uniforms(ct.SEED, ct.BASE, B, N, ct.OFFSET, ct.K)
    assert u.min() >= 0.0 and u.max() < 1.0
    idx, _, margin = ct.pick(lg, u)
    assert set(np.unique(idx).tolist()) == {0, 1, 2, 3, 4}
    # the exempt share of the fp64 reference alone, at the band the GPU test uses: at most 2 % of the rows
    share = float(ct.exempt(margin, beta).mean())
    assert share <= 0.02, share
    # the torch fp32 actor against the fp64 one: rows outside the band pick the same index
    a32 = ct.cat_actor(fam, N, H, seed=ct.case_seed(fam, N, B, H))
    for k in range(ct.K):
        obs = ct.cpu_observations(N, B, seed=1 + k)
        h = (torch.rand(B, N, H, dtype=torch.float64, generator=torch.Generator().manual_seed(k)) - 0.5) if fam == "gru" else None
        with torch.no_grad():
            l32 = a32.logits(obs.float(), h.float())[0] if fam == "gru" else a32.logits(obs.float())
        i32 = ct.pick(l32.double().numpy(), u[k])[0]
        keep = ~ct.exempt(margin[k], beta[k])
        assert np.array_equal(i32[keep], idx[k][keep])
    p = np.exp(lg - lg.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    redraw = float((1.0 - (p * p).sum(-1)).mean())                                 # two independent draws pick different indices
    off_mode = float((1.0 - p.max(-1)).mean())                                     # a sample is not the mode
    assert redraw >= 0.15 and off_mode >= 0.1, (redraw, off_mode)
    for mode in (ct.ONEHOT5, ct.INDEX):
        sh = _mutant_shares(lg, N, B, mode)
        for m in ("word0", "word3", "base_dropped"):
            assert sh[m]["u"] >= 0.99 and sh[m]["idx"] >= 0.8 * redraw, (m, sh[m], redraw)
        assert sh["offset_not_advanced"]["u"] >= 0.99 * 2 / 3 and sh["offset_not_advanced"]["idx"] >= 0.8 * redraw * 2 / 3
        assert sh["t_is_u"]["idx"] >= 0.1 and sh["descending_cumsum"]["idx"] >= 0.1
        for m in ("modes_swapped", "axes_swapped"):
            assert sh[m]["idx"] == 0.0 and sh[m]["act"] == sh[m]["moved"] >= 0.5, (m, sh[m])
        assert sh["logp_of_greedy"]["idx"] == 0.0 and sh["logp_of_greedy"]["logp"] >= 0.8 * off_mode
        assert sh["greedy_highest_tie"] == dict(sh["greedy_highest_tie"], u=0.0, idx=0.0, act=0.0, logp=0.0)   # ties only: below


def test_tie_mutant_and_edge_rows_of_the_standalone_inputs():
    lg, u = ct.standalone_inputs()
    l64 = lg.astype(np.float64)
    g, glp, _ = ct.pick(l64, greedy=True)
    gm = ct.pick(l64, greedy=True, mutant="greedy_highest_tie")[0]
    rows = np.arange(len(lg))
    tied = (rows % 64 == 0) | (rows % 64 == 2) | (rows % 64 == 3)
    assert np.array_equal(g != gm, tied)                                       # exactly the tied rows: share 1 there, 0 elsewhere
    assert bool((g[rows % 64 == 0] == 0).all()) and bool((g[rows % 64 == 2] == 1).all()) and bool((g[rows % 64 == 3] == 0).all())
    idx, logp, margin = ct.pick(l64, u.astype(np.float64))
    one = rows % 64 == 1
    assert bool((idx[one & (u > 0)] == 3).all()) and np.allclose(logp[one & (u > 0)], 0.0)    # underflowing classes: never sampled
    assert bool((margin[one & (u == 0)] < ct.ETA0).all())    # ... but u = 0 sits on fp64's boundary c_0 = e^-200: an exempt row
    e0 = np.exp(l64[:, 0] - l64.max(-1))
    assert bool((idx[(u == 0) & (e0 > 0)] == 0).all())                         # t = 0 < c_0 wherever class 0 has any mass
    top = np.float32(1.0 - 2.0 ** -24)
    assert bool((u[1::5] == top).all()) and bool((idx[(u == top) & (rows % 64 == 0)] == 4).all())   # the largest u, equal logits
    assert bool(np.isfinite(logp).all()) and set(np.unique(idx).tolist()) == {0, 1, 2, 3, 4}
    assert float(ct.exempt(margin, 0.0).mean()) < 0.3                          # u = 0 rows sit on no boundary; most rows count
