"""CPU checks of the 16-bit members of the fused actor launch (`fg_rollout_hd_actor_obs16`, `fg_rollout_hd_actor_cat_obs16`): the
symbols, the dry runs' 36 instantiations and their resources, argument checks that touch no device, the fp32 dry runs left alone,
and which route `env.obs_path(dtype, actor=...)` answers on a stand-in env."""
import ctypes
import os
import re
import types

import pytest
import torch

from formation_gym import GaussianActor, OUNoiseActor, PerAgentActor, _native, load_scenario
from formation_gym.environment import MultiAgentEnv
from tests import actor_cat_testlib as ct
from tests.actor_testlib import ROOT, fake_actor, params as _params

from . import isa_scan

ENTRIES = ("fg_rollout_hd_actor_obs16", "fg_rollout_hd_actor_cat_obs16", "fg_describe_actor_obs16_launch",
           "fg_describe_actor_cat_obs16_launch")
GAUSS, CAT = "fg_rollout_hd_actor_obs16", "fg_rollout_hd_actor_cat_obs16"
FORMATS = (_native.FG_OBS_F16, _native.FG_OBS_BF16)
FUSED_N, FUSED_H = (3, 9, 27), (32, 64)
FAMILIES = ("plain", "ln", "gru")
# (16-bit kernel, its fp32 twin, the twin's dry run) by (kind, family)
KERNELS = {("gauss", "plain"): ("actor_sample_obs16", "actor_sample_kernel"), ("gauss", "ln"): ("ln_sample_obs16", "ln_sample_kernel"),
           ("gauss", "gru"): ("gru_sample_obs16", "gru_sample_kernel"), ("cat", "plain"): ("cat_actor_obs16", "cat_actor_kernel"),
           ("cat", "ln"): ("ln_cat_actor_obs16", "ln_cat_actor_kernel"), ("cat", "gru"): ("gru_cat_actor_obs16", "gru_cat_actor_kernel")}
ONEHOT5, INDEX = _native.FG_ACT_ONEHOT5, _native.FG_ACT_INDEX
P = 4096                                                   # a stand-in address: only NULL-ness and alignment are looked at
LOG_STD = ctypes.c_void_p(P)


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def _norm(**kw):
    d = dict(in_gamma=P, in_beta=P, h1_gamma=P, h1_beta=P, h2_gamma=P, h2_beta=P, in_eps=1e-5, h1_eps=1e-5, h2_eps=1e-5, in_norm=1)
    d.update(kw)
    return _native.FgActorNorm(**d)


def _gru(**kw):
    d = dict(w_ih=P, w_hh=P, b_ih=P, b_hh=P, norm_gamma=P, norm_beta=P, norm_eps=1e-5)
    d.update(kw)
    return _native.FgActorGru(**d)


def _call(lib, kind, dry, fam="plain", fmt=_native.FG_OBS_F16, N=9, K=20, B=128, H=64, tanh=0, params=None, log_std=LOG_STD,
          mode=ONEHOT5, greedy=0, obs=P, idx=P, logp=P, state=P, states=None, every=1, norm="fake", gru="fake", actor="fake"):
    """(status, fg_last_error(), text) of the Gaussian (`kind` 'gauss') or categorical 16-bit entry - its dry run when `dry` - on
    stand-in pointers."""
    fa = fake_actor(H, tanh) if actor == "fake" else actor
    fn = None if fam == "plain" else (_norm() if norm == "fake" else norm)
    fg = None if fam != "gru" else (_gru() if gru == "fake" else gru)
    lead = (params or _params(), fmt, fa, fn, fg) + ((log_std,) if kind == "gauss" else (mode, greedy))
    text = ""
    if dry:
        buf = ctypes.create_string_buffer(512)
        fn_ = lib.fg_describe_actor_obs16_launch if kind == "gauss" else lib.fg_describe_actor_cat_obs16_launch
        rc = fn_(*lead, B, N, K, 1, buf, 512)
        text = buf.value.decode()
    else:
        bufs = [P] * 8 + [obs] + [P] * 3                   # the state's eight, obs_seq, reward_seq, indiv_seq, done_seq
        if kind == "gauss":
            rc = lib.fg_rollout_hd_actor_obs16(*lead, B, N, K, *bufs, logp, state, states, every, 1, None)
        else:
            rc = lib.fg_rollout_hd_actor_cat_obs16(*lead, B, N, K, *bufs, idx, logp, state, states, every, 1, None)
    return rc, lib.fg_last_error().decode(), text


def test_symbols_exported_declared_and_bound(lib):
    raw = ctypes.CDLL(_native.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "formation_hip.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ENTRIES:
        assert hasattr(raw, name) and name in _native.SIGNATURES and ("int %s(" % name) in header and name in doc, name
    assert lib.fg_abi_version() == _native.ABI_VERSION == 8                            # an additive change


def test_describe_names_36_instantiations_that_are_in_the_library(lib):
    names = {}
    B = 1000
    for (kind, fam), (k16, k32) in KERNELS.items():
        for N in FUSED_N:
            for H in FUSED_H:
                texts = {_call(lib, kind, True, fam, fmt=fmt, N=N, H=H, B=B, mode=mode, greedy=greedy)
                         for fmt in FORMATS for mode in (ONEHOT5, INDEX) for greedy in (0, 1)}
                assert len(texts) == 1, texts                                          # the format (mode, flag) picks no kernel
                rc, err, text = texts.pop()
                assert rc == 0, (kind, fam, N, H, err)
                E = 256 // (4 if N <= 4 else 16 if N <= 16 else 32)
                m = re.fullmatch(r"%s<%d,%d> grid (\d+) block 256 envs/wg %d lds (\d+); " % (k16, N, H, E), text)
                assert m, text
                assert int(m.group(1)) == -(-B // E)
                assert 0 < int(m.group(2)) <= 160 * 1024
                names["fg::%s<%d, %d>(" % (k16, N, H)] = (kind, fam, N, H, text)
    assert len(names) == 6 * len(FUSED_N) * len(FUSED_H) == 36
    built = isa_scan.kernel_resources(_native.LIB_PATH)
    for n in names:
        hit = [k for k in built if k["demangled"].startswith("void " + n)]
        assert len(hit) == 1, n
        k = hit[0]
        assert k["private_segment"] == 0 and k["vgpr_spill"] == 0, (n, k)
    # no instantiation besides these: every kernel of the six names is one the dry runs named
    for k in built:
        m = re.match(r"void (fg::(\w+)<\d+, \d+>\()", k["demangled"])
        if m and m.group(2) in {v[0] for v in KERNELS.values()}:
            assert m.group(1) in names, k["demangled"]


def test_the_tiles_share_the_fp32_twins_lds_and_the_fp32_dry_runs_answer_as_before(lib):
    """The 16-bit tiles live in the waves' activation tiles, so a member's LDS is its fp32 twin's; the fp32 entries' dry runs name
    the kernels they named before, with the geometry the 16-bit one reports."""
    B = 4096
    for (kind, fam), (k16, k32) in KERNELS.items():
        for N in FUSED_N:
            for H in FUSED_H:
                fa, fn, fg = fake_actor(H, 0), (None if fam == "plain" else _norm()), (_gru() if fam == "gru" else None)
                buf = ctypes.create_string_buffer(512)
                tail = (B, N, 20, 1, buf, 512)
                if kind == "cat":
                    rc = lib.fg_describe_actor_cat_launch(_params(), fa, fn, fg, ONEHOT5, 0, *tail)
                elif fam == "plain":
                    rc = lib.fg_describe_actor_sample_launch(_params(), fa, LOG_STD, *tail)
                elif fam == "ln":
                    rc = lib.fg_describe_actor_norm_launch(_params(), fa, fn, LOG_STD, *tail)
                else:
                    rc = lib.fg_describe_actor_gru_launch(_params(), fa, fn, fg, LOG_STD, *tail)
                assert rc == 0, (kind, fam, N, H)
                text32 = buf.value.decode()
                assert text32.startswith("%s<%d,%d> grid " % (k32, N, H)), text32
                text16 = _call(lib, kind, True, fam, N=N, H=H, B=B)[2]
                assert text16 == text32.replace(k32 + "<", k16 + "<", 1), (text16, text32)


@pytest.mark.parametrize("kind", ["gauss", "cat"])
def test_status_codes_without_a_device(lib, kind):
    who = GAUSS if kind == "gauss" else CAT
    OK, BAD, UNSUP, ALIGN = _native.FG_OK, _native.FG_ERR_BAD_ARG, _native.FG_ERR_UNSUPPORTED_N, _native.FG_ERR_ALIGNMENT
    for dry in (False, True):
        for fam in FAMILIES:
            bad = lambda **kw: _call(lib, kind, dry, fam, **kw)[:2]
            # the members' own checks, in their order and in the entry's name
            for fmt in (0, 3, -1):
                assert bad(fmt=fmt) == (BAD, who + ": obs_format must be FG_OBS_F16 or FG_OBS_BF16"), fmt
                assert bad(fmt=fmt, N=4)[0] == BAD                                     # ... before the agent count
            p = _params(); p.obs_env_pitch = 512
            assert bad(params=p) == (BAD, who + ": a padded env pitch (obs_env_pitch) is not supported")
            assert bad(params=p, N=4)[0] == BAD
            if kind == "gauss":
                assert bad(log_std=None) == (BAD, who + ": log_std is NULL")
                assert bad(log_std=None, N=4)[0] == BAD
            for N in (4, 8, 16, 25, 32, 5, 81):
                assert bad(N=N) == (UNSUP, who + ": N must be 3, 9 or 27"), N
            assert bad(N=4, H=128)[0] == UNSUP                                         # ... before the width
            assert bad(H=128) == (BAD, who + ": hidden must be 32 or 64")
            # then the fp32 entries' checks, with their texts
            assert bad(H=48) == (BAD, "fg_rollout_hd_actor: hidden must be 32, 64 or 128")
            assert bad(K=0)[0] == BAD and bad(actor=None)[0] == BAD and bad(B=-1)[0] == BAD
            for opt in ("u_noise", "max_speed", "accel"):
                p = _params(); setattr(p, opt, 0.5)
                assert bad(params=p)[0] == BAD, opt
            if fam != "plain":
                assert bad(norm=_norm(h1_eps=0.0)) == (BAD, who + ": h1_eps must be positive and finite")
            if fam == "gru":
                assert bad(gru=_gru(w_hh=None)) == (BAD, who + ": w_hh is NULL")
                assert bad(gru=_gru(b_ih=P + 2)) == (ALIGN, who + ": b_ih must be 4-byte aligned")
            if kind == "cat":
                assert bad(tanh=1) == (BAD, who + ": out_tanh must be 0: the head's outputs are logits")
                assert bad(mode=_native.FG_ACT_ARGMAX) == (BAD, who + ": act_mode must be FG_ACT_ONEHOT5 or FG_ACT_INDEX")
            else:
                assert bad(log_std=ctypes.c_void_p(P + 2))[0] == ALIGN
    # gru without norm
    rc, err, _ = _call(lib, kind, True, "gru", norm=None)
    assert (rc, err) == (BAD, who + ": norm is NULL")
    # the launch's own buffers, after every check above
    for fam in FAMILIES:
        bad = lambda **kw: _call(lib, kind, False, fam, **kw)[:2]
        rc, err = bad(obs=P + 4)
        assert rc == ALIGN and "obs_seq must be 16-byte" in err
        assert bad(obs=P + 8)[0] == ALIGN
        assert bad(logp=P + 1)[0] == ALIGN
        if kind == "cat":
            assert bad(idx=None) == (BAD, who + ": idx_seq is NULL")
        assert bad(B=0)[0] == OK and bad(B=0, obs=None, idx=None, logp=None, state=None)[0] == OK      # no launch ...
        assert bad(B=0, fmt=0)[0] == BAD and bad(B=0, N=4)[0] == UNSUP and bad(B=0, H=128)[0] == BAD    # ... after the checks
    bad = lambda **kw: _call(lib, kind, False, "gru", **kw)[:2]
    assert bad(state=None) == (BAD, who + ": rnn_state is NULL")
    assert bad(state=P + 8)[0] == ALIGN
    assert bad(states=P, every=0) == (BAD, who + ": states_every >= 1 required")
    assert bad(states=P + 8, every=2) == (ALIGN, who + ": rnn_states must be 16-byte aligned")
    assert _call(lib, kind, True, B=0)[0] == BAD

# ---- env.obs_path(dtype, actor=...) on a stand-in env: the scenario object, a world that answers what `Scenario.params` and
# `_resolve_actor` ask, the env's own resolution - no device ----
def _standin(name, N, mode=0, **options):
    sc = load_scenario(name)
    sc._seed = 1

    def native_params(**kw):
        p = _params(dist_min=0.03, collide_thresh=kw.get("collide_thresh", 0.015))
        for k, v in options.items():
            setattr(p, k, v)
        return p
    world = types.SimpleNamespace(agents=[types.SimpleNamespace(size=0.03) for _ in range(N)], num_envs=64, dim_c=2,
                                  device=torch.device("cpu"), any_non_silent=lambda: False, native_params=native_params)
    env = types.SimpleNamespace(scenario=sc, world=world, post_step_callback=None, num_agents=N, _action_mode=lambda: mode)
    env._actor_facts = lambda: MultiAgentEnv._actor_facts(env)
    env._resolve_actor = lambda actor: MultiAgentEnv._resolve_actor(env, actor)
    return env


def _path(env, dtype, actor):
    return MultiAgentEnv.obs_path(env, dtype, actor=actor)


def _gauss(fam, N, H):
    return GaussianActor(ct.cat_actor(fam, N, H, head=2).logits)


def _mlp(N, H):
    nn = torch.nn
    return nn.Sequential(nn.Linear(6 * N, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 2))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_obs_path_with_an_actor(lib, dtype):
    cont, disc = _standin("formation_hd_env", 9), _standin("formation_hd_env", 9, mode=ONEHOT5)
    for fam in FAMILIES:
        for H in FUSED_H:
            assert _path(cont, dtype, _gauss(fam, 9, H)) == "fused", (fam, H)
            assert _path(disc, dtype, ct.cat_actor(fam, 9, H)) == "fused", (fam, H)
    for N in FUSED_N:
        assert _path(_standin("formation_hd_env", N), dtype, _gauss("ln", N, 64)) == "fused", N
    casts = {"a deterministic MLP": _mlp(9, 64), "OU noise": OUNoiseActor(_mlp(9, 64)),
             "per-agent": GaussianActor(PerAgentActor([_mlp(9, 32) for _ in range(9)])), "H = 128": GaussianActor(_mlp(9, 128)),
             "a callable": lambda obs: obs[..., :2]}
    for what, actor in casts.items():
        assert _path(cont, dtype, actor) == "cast", what
    assert _path(_standin("formation_hd_env", 4), dtype, _gauss("ln", 4, 64)) == "cast"
    assert _path(_standin("formation_hd_env", 9, u_noise=0.1), dtype, _gauss("ln", 9, 64)) == "cast"     # a World option
    assert _path(_standin("basic_formation_env", 3), dtype, GaussianActor(_mlp(2, 32))) == "cast"        # a landmark scenario
    cb = _standin("formation_hd_env", 9)
    cb.post_step_callback = lambda world: None                                         # a host function after every step
    assert _path(cb, dtype, _gauss("ln", 9, 64)) == "cast"
    # without an actor the answer is the open-loop launch's, as before
    assert MultiAgentEnv.obs_path(cont, dtype) == "fused" and MultiAgentEnv.obs_path(cont, dtype, True) == "fused"


def test_obs_dtype_must_be_a_16_bit_float():
    env = _standin("formation_hd_env", 9)
    for bad in (None, torch.float32, torch.float64):
        with pytest.raises(ValueError):
            _path(env, bad, _gauss("ln", 9, 32))
