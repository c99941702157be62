"""CPU checks of the LayerNorm actor rollout (`fg_rollout_hd_actor_norm`, ln_actor_kernel / ln_sample_kernel): which path a
LayerNorm actor takes, what `resolve_actor` hands to the launch, the dry-run description, argument checks that touch no
device, and the new kernels' resources next to the unchanged counts of the existing actor kernel families."""
import ctypes
import os
import types

import pytest
import torch

from formation_gym import GaussianActor, PerAgentActor, _native, load_scenario
from formation_gym.actor_rollout import (FUSED_HIDDEN, FUSED_LN_HIDDEN, FUSED_N, FusedActor, actor_path, actor_spec,
                                         layernorm_spec, resolve_actor)
from tests.actor_testlib import LIB, ROOT, describe, fake_actor as _fake_actor, fake_actors, params as _params

nn = torch.nn


def _ln_mlp(N, H, in_norm=True, tanh=False, bias=True, affine=True, eps=1e-5, D=None):
    D = 6 * N if D is None else D
    mods = [nn.LayerNorm(D, eps=eps, elementwise_affine=affine)] if in_norm else []
    mods += [nn.Linear(D, H, bias=bias), nn.ReLU(), nn.LayerNorm(H, eps=eps, elementwise_affine=affine),
             nn.Linear(H, H, bias=bias), nn.ReLU(), nn.LayerNorm(H, eps=eps, elementwise_affine=affine), nn.Linear(H, 2, bias=bias)]
    if tanh:
        mods.append(nn.Tanh())
    return nn.Sequential(*mods)


def _plain_mlp(N, H, tanh=False):
    mods = [nn.Linear(6 * N, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 2)]
    return nn.Sequential(*(mods + [nn.Tanh()] if tanh else mods))


def test_fused_ln_hidden_is_its_own_constant():
    assert tuple(FUSED_LN_HIDDEN) == (32, 64) and set(FUSED_LN_HIDDEN) < set(FUSED_HIDDEN)


@pytest.mark.parametrize("H", FUSED_LN_HIDDEN)
def test_layernorm_actor_fuses(H):
    for N in FUSED_N:
        for in_norm in (True, False):
            for tanh in (True, False):
                actor = _ln_mlp(N, H, in_norm, tanh)
                assert actor_path(actor, N) == "fused", (N, in_norm, tanh)
                assert actor_path(GaussianActor(actor), N) == "fused", (N, in_norm, tanh)
    N = 9
    assert actor_path(_ln_mlp(N, H, bias=False), N) == "fused"                     # bias-free Linears
    assert actor_path(_ln_mlp(N, H, affine=False), N) == "fused"                   # affine-free norms
    assert actor_path(_ln_mlp(N, H, eps=3e-3), N) == "fused"                       # a non-default eps
    nobias = _ln_mlp(N, H)
    nobias[3] = nn.LayerNorm(H, bias=False)                                        # gamma without beta
    assert actor_path(nobias, N) == "fused" and resolve_actor(nobias, N).norms.hidden1[1] is None


def test_resolve_hands_back_the_norm_tensors_themselves():
    N, H = 9, 64
    actor = _ln_mlp(N, H, eps=2e-4)
    actor[6].eps = 7e-6
    fa = resolve_actor(actor, N)
    assert isinstance(fa, FusedActor) and (fa.hidden, fa.out_tanh, fa.per_agent, fa.log_std) == (H, False, False, None)
    ws = fa.members[0]
    for got, want in zip(ws, (actor[1].weight, actor[1].bias, actor[4].weight, actor[4].bias, actor[7].weight, actor[7].bias)):
        assert got is want
    n0, n1, n2 = fa.norms
    assert n0[0] is actor[0].weight and n0[1] is actor[0].bias and n0[2] == 2e-4
    assert n1[0] is actor[3].weight and n1[1] is actor[3].bias and n1[2] == 2e-4
    assert n2[0] is actor[6].weight and n2[1] is actor[6].bias and n2[2] == 7e-6
    # without the input norm, and without affine parameters
    fb = resolve_actor(_ln_mlp(N, H, in_norm=False, affine=False, tanh=True), N)
    assert fb.out_tanh and fb.norms.input is None and fb.norms.hidden1[:2] == (None, None) and fb.norms.hidden2[:2] == (None, None)
    # as a GaussianActor's mean: the same record with its log_std
    g = GaussianActor(actor)
    fg = resolve_actor(g, N)
    assert fg.log_std is g.log_std and fg.norms.hidden2[0] is actor[6].weight and fg.members[0][0] is actor[1].weight
    # the ctypes struct the launch takes
    s = _native.actor_norm(fa.norms)
    assert s.in_norm == 1 and s.in_gamma == actor[0].weight.data_ptr() and s.h2_beta == actor[6].bias.data_ptr()
    assert abs(s.in_eps - 2e-4) < 1e-10 and abs(s.h2_eps - 7e-6) < 1e-12
    s = _native.actor_norm(fb.norms)
    assert s.in_norm == 0 and not s.in_gamma and not s.h1_gamma and not s.h2_beta


def test_actor_without_norms_resolves_as_before():
    N = 9
    for H in FUSED_HIDDEN:
        m = _plain_mlp(N, H, tanh=True)
        fa = resolve_actor(m, N)
        want = FusedActor(H, True, [[m[0].weight, m[0].bias, m[2].weight, m[2].bias, m[4].weight, m[4].bias]], False, None)
        assert fa.norms is None and fa[:2] == want[:2] and fa[3:] == want[3:]
        assert all(a is b for a, b in zip(fa.members[0], want.members[0])) and len(fa.members) == 1
        assert layernorm_spec(m, N) is None
        hidden, out_tanh, ws = actor_spec(m, N)                                    # the tuple keeps its shape
        assert (hidden, out_tanh) == (H, True) and len(ws) == 6
    g = GaussianActor(_plain_mlp(N, 128))
    fg = resolve_actor(g, N)
    assert fg.norms is None and fg.hidden == 128 and fg.log_std is g.log_std
    pa = resolve_actor(PerAgentActor([_plain_mlp(N, 64) for _ in range(N)]), N)
    assert pa.norms is None and pa.per_agent and len(pa.members) == N
    assert actor_spec(_ln_mlp(N, 64), N) is None                                   # actor_spec never takes a LayerNorm


def test_layernorm_actor_host_paced():
    N, H = 9, 64
    assert actor_path(_ln_mlp(N, 128), N) == "host"                               # H = 128 with norms
    assert actor_path(GaussianActor(_ln_mlp(N, 128)), N) == "host"
    assert actor_path(_ln_mlp(N, 48), N) == "host"
    one = _ln_mlp(N, H)
    del one[6]                                                                     # one hidden norm only
    assert [type(m) for m in one].count(nn.LayerNorm) == 2 and actor_path(one, N) == "host"
    first_only = nn.Sequential(nn.Linear(54, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.LayerNorm(H), nn.Linear(H, 2))
    assert actor_path(first_only, N) == "host"
    lead_only = nn.Sequential(nn.LayerNorm(54), *_plain_mlp(N, H))                 # the input norm without the hidden ones
    assert actor_path(lead_only, N) == "host"
    pre = nn.Sequential(nn.Linear(54, H), nn.LayerNorm(H), nn.ReLU(), nn.Linear(H, H), nn.LayerNorm(H), nn.ReLU(),
                        nn.Linear(H, 2))                                           # norms before the ReLU
    assert actor_path(pre, N) == "host"
    wrong = _ln_mlp(N, H)
    wrong[3] = nn.LayerNorm(H // 2)                                                # a wrong normalized_shape
    assert actor_path(wrong, N) == "host"
    wrong_in = _ln_mlp(N, H)
    wrong_in[0] = nn.LayerNorm(6 * N + 2)
    assert actor_path(wrong_in, N) == "host"
    two_axes = _ln_mlp(N, H)
    two_axes[0] = nn.LayerNorm((N, 6 * N))                                         # over more than the last axis
    assert actor_path(two_axes, N) == "host"
    f64 = _ln_mlp(N, H)
    f64[6] = nn.LayerNorm(H).double()                                              # fp64 norm parameters
    assert actor_path(f64, N) == "host"
    strided = _ln_mlp(N, H)
    strided[3].weight = nn.Parameter(torch.ones(2 * H)[::2])                       # non-contiguous gamma
    assert not strided[3].weight.is_contiguous() and actor_path(strided, N) == "host"
    strided_b = _ln_mlp(N, H)
    strided_b[0].bias = nn.Parameter(torch.zeros(12 * N)[::2])
    assert actor_path(strided_b, N) == "host"
    bad_eps = _ln_mlp(N, H)
    bad_eps[3].eps = 0.0
    assert actor_path(bad_eps, N) == "host"
    good = _ln_mlp(N, H)
    assert actor_path(good, N) == "fused"
    assert actor_path(good, N, device="cuda:0") == "host"                          # parameters off the env's device
    assert actor_path(GaussianActor(good), N, device="cuda:0") == "host"
    assert actor_path(good, 81) == "host" and actor_path(good, 10) == "host"       # N outside FUSED_N
    # PerAgentActor members with norms
    assert actor_path(PerAgentActor([_ln_mlp(N, H) for _ in range(N)]), N) == "host"
    assert actor_path(GaussianActor(PerAgentActor([_ln_mlp(N, H) for _ in range(N)])), N) == "host"
    # the env's facts
    for g in (good, GaussianActor(good)):
        assert actor_path(g, N, world_options=True) == "host"
        assert actor_path(g, N, callback=True) == "host"
        assert actor_path(g, N, silent=False) == "host"
        assert actor_path(g, N, continuous=False) == "host"
        assert actor_path(g, N, fused_scenario=False) == "host"
    # a GaussianActor whose log_std the launch cannot read
    g = GaussianActor(good)
    g.log_std = nn.Parameter(torch.zeros(2, dtype=torch.float64))
    assert actor_path(g, N) == "host"


@pytest.mark.parametrize("name,N,L,M,num_obs,D", [("basic_formation_env", 3, 3, 0, 0, 18),
                                                  ("formation_hd_partial_env", 5, 5, 0, 3, 26),
                                                  ("formation_hd_obs_env", 4, 4, 3, 0, 28)])
def test_landmark_scenarios_run_layernorm_actors_host_paced(name, N, L, M, num_obs, D):
    sc = load_scenario(name)
    world = types.SimpleNamespace(agents=[None] * N, landmarks=[None] * (L + M))
    sc.num_agents, sc.num_landmarks, sc.num_obstacles, sc.num_obs, sc.obs_range = N, L, M, num_obs, 0.0
    facts = sc.actor_fused_rule(world)
    assert facts["fused_ln_hidden"] == () and facts["per_agent"] is False          # the rule states it with a fact
    for H in (32, 64):
        ln = _ln_mlp(N, H, D=D)
        assert actor_path(ln, N, fused_scenario=True, **facts) == "host"
        assert actor_path(GaussianActor(ln), N, fused_scenario=True, **facts) == "host"
        assert actor_path(_ln_mlp(N, H, in_norm=False, D=D), N, fused_scenario=True, **facts) == "host"
        plain = nn.Sequential(nn.Linear(D, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 2))
        assert actor_path(plain, N, fused_scenario=True, **facts) == "fused"       # the plain body still fuses there


# ---- the C ABI without a device ----


def _fake_norm(in_norm=1, eps=1e-5, **kw):
    addr = 4096
    d = dict(in_gamma=addr, in_beta=addr, h1_gamma=addr, h1_beta=addr, h2_gamma=addr, h2_beta=addr, in_eps=eps, h1_eps=eps,
             h2_eps=eps, in_norm=in_norm)
    d.update(kw)
    return _native.FgActorNorm(**d)


def _describe(lib, N, H, sample, norm="default", B=4096, K=20):
    norm = _fake_norm() if norm == "default" else norm
    return describe(lib, "fg_describe_actor_norm_launch", (_fake_actor(H), norm, 4096 if sample else None), N, B, K)


def test_struct_layout_matches_the_header(tmp_path):
    import subprocess
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "formation_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(FgActorNorm));']
    for fname, _ in _native.FgActorNorm._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(FgActorNorm, %s));' % (fname, fname))
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(_native.FgActorNorm)
    for fname, _ in _native.FgActorNorm._fields_:
        assert int(got[fname]) == getattr(_native.FgActorNorm, fname).offset, fname
    assert _native.load().fg_abi_version() == 8                                    # an additive change


def test_describe_names_one_instantiation_per_shape():
    lib = _native.load()
    names = set()
    for N in FUSED_N:
        for H in FUSED_LN_HIDDEN:
            for sample in (False, True):
                kernel = "ln_sample_kernel" if sample else "ln_actor_kernel"
                for in_norm in (1, 0):                                             # a run-time fact: the same instantiation
                    rc, text = _describe(lib, N, H, sample, _fake_norm(in_norm))
                    assert rc == 0, text
                    assert text.count(kernel + "<") == 1 and "%s<%d,%d>" % (kernel, N, H) in text, text
                    assert text.count("_kernel<") == 1, text
                    assert " grid " in text and " lds " in text
                    names.add(text.split(" ")[0])
                    lds = int(text.split(" lds ")[1].split(";")[0])
                    assert lds <= 160 * 1024
    assert len(names) == 2 * len(FUSED_N) * len(FUSED_LN_HIDDEN)


def test_bad_arguments_rejected_without_a_device():
    lib = _native.load()
    f = ctypes.c_void_p(4096)

    def call(N=9, K=20, H=64, norm="default", log_std=4096, logp=4096):
        norm = _fake_norm() if norm == "default" else norm
        return lib.fg_rollout_hd_actor_norm(_params(), _fake_actor(H), norm, log_std, 128, N, K, *([f] * 12), logp, 1, None)
    assert call(H=128) == -1 and b"hidden" in lib.fg_last_error()
    assert call(H=48) == -1
    assert call(N=81) == -2
    assert call(norm=None) == -1 and b"norm is NULL" in lib.fg_last_error()
    assert call(norm=_fake_norm(eps=0.0)) == -1 and b"eps" in lib.fg_last_error()
    assert call(norm=_fake_norm(h1_eps=0.0)) == -1 and b"h1_eps" in lib.fg_last_error()
    assert call(norm=_fake_norm(h2_eps=float("inf"))) == -1 and b"h2_eps" in lib.fg_last_error()
    assert call(norm=_fake_norm(h2_eps=float("nan"))) == -1
    assert call(norm=_fake_norm(in_eps=-1.0)) == -1 and b"in_eps" in lib.fg_last_error()
    assert call(norm=_fake_norm(h1_beta=4098)) == -1 and b"h1_beta" in lib.fg_last_error()
    assert call(norm=_fake_norm(in_gamma=4097)) == -1 and b"in_gamma" in lib.fg_last_error()
    assert call(K=0) == -1
    assert call(log_std=4098) == -3 and call(logp=4098) == -3                      # as fg_rollout_hd_actor_sample
    for sample in (False, True):                                                   # the dry run makes the same checks
        assert _describe(lib, 9, 128, sample)[0] == -1
        assert _describe(lib, 81, 64, sample)[0] == -2
        assert _describe(lib, 9, 64, sample, norm=None)[0] == -1
        assert _describe(lib, 9, 64, sample, norm=_fake_norm(eps=0.0))[0] == -1
        assert _describe(lib, 9, 64, sample, B=0)[0] == -1


# ---- the eight hd-actor entry points: every failing check's status and fg_last_error() text, and the order of the checks ----
HD_ACTOR_ENTRIES = {"shared": ("fg_rollout_hd_actor", "fg_describe_actor_launch"),
                    "sample": ("fg_rollout_hd_actor_sample", "fg_describe_actor_sample_launch"),
                    "per_agent": ("fg_rollout_hd_actor_per_agent", "fg_describe_actor_per_agent_launch"),
                    "norm": ("fg_rollout_hd_actor_norm", "fg_describe_actor_norm_launch")}
_ALL, _ONE, _PA, _LN = tuple(HD_ACTOR_ENTRIES), ("shared", "sample", "norm"), ("per_agent",), ("norm",)
_GAUSS, _RUN, _DRY, _BOTH = ("sample", "per_agent", "norm"), (False,), (True,), (False, True)
_N_LIST = "N must be 3, 4, 8, 9, 16, 25, 27 or 32"
# (entries, the rollout entry and / or its describe twin, what is wrong with the call, status, fg_last_error()); a text of None:
# the call succeeds.  The literals are the answers of the library before the entries shared one check-and-run.
HD_ACTOR_BAD_CALLS = [
    (_ONE, _BOTH, dict(actor=None), -1, "fg_rollout_hd_actor: actor is NULL"),
    (_PA, _BOTH, dict(actor=None), -1, "fg_rollout_hd_actor_per_agent: actors is NULL"),
    (_ALL, _BOTH, dict(H=48), -1, "fg_rollout_hd_actor: hidden must be 32, 64 or 128"),
    (_ONE, _BOTH, dict(N=81), -2, "fg_rollout_hd_actor: " + _N_LIST),
    (_PA, _BOTH, dict(N=81), -2, "fg_rollout_hd_actor_per_agent: " + _N_LIST),
    (_ONE, _BOTH, dict(K=0), -1, "fg_rollout_hd_actor: B >= 0 and K >= 1 required"),
    (_PA, _BOTH, dict(K=0), -1, "fg_rollout_hd_actor_per_agent: B >= 0 and K >= 1 required"),
    (_ONE, _BOTH, dict(B=-1), -1, "fg_rollout_hd_actor: B >= 0 and K >= 1 required"),
    (_PA, _BOTH, dict(B=-1), -1, "fg_rollout_hd_actor_per_agent: B >= 0 and K >= 1 required"),
    (_ONE, _BOTH, dict(N=81, H=48), -2, "fg_rollout_hd_actor: " + _N_LIST),                         # N before the actor
    (_PA, _BOTH, dict(N=81, H=48), -2, "fg_rollout_hd_actor_per_agent: " + _N_LIST),
    (_ONE, _BOTH, dict(K=0, N=81), -1, "fg_rollout_hd_actor: B >= 0 and K >= 1 required"),          # B and K before N
    (_PA, _BOTH, dict(K=0, N=81), -1, "fg_rollout_hd_actor_per_agent: B >= 0 and K >= 1 required"),
    (_LN, _BOTH, dict(H=128), -1, "fg_rollout_hd_actor_norm: hidden must be 32 or 64 with LayerNorms"),
    (_LN, _BOTH, dict(H=128, norm=None), -1, "fg_rollout_hd_actor_norm: norm is NULL"),             # norm before hidden
    (_LN, _BOTH, dict(H=128, log_std=4098), -1, "fg_rollout_hd_actor_norm: hidden must be 32 or 64 with LayerNorms"),
    (_LN, _BOTH, dict(norm=None), -1, "fg_rollout_hd_actor_norm: norm is NULL"),
    (_LN, _BOTH, dict(norm=dict(h1_eps=0.0)), -1, "fg_rollout_hd_actor_norm: h1_eps must be positive and finite"),
    (_LN, _BOTH, dict(norm=dict(h1_eps=0.0, h2_beta=4098)), -1, "fg_rollout_hd_actor_norm: h1_eps must be positive and finite"),
    (_LN, _BOTH, dict(norm=dict(h2_beta=4098)), -1, "fg_rollout_hd_actor_norm: h2_beta must be 4-byte aligned"),
    (_LN, _BOTH, dict(norm=dict(h2_beta=4098), log_std=4098), -1, "fg_rollout_hd_actor_norm: h2_beta must be 4-byte aligned"),
    (_PA, _BOTH, dict(member=(3, 32)), -1, "fg_rollout_hd_actor_per_agent: member 3 differs from member 0 in hidden or out_tanh"),
    (_PA, _BOTH, dict(member=(3, 48)), -1, "fg_rollout_hd_actor: hidden must be 32, 64 or 128"),    # a member's own checks first
    (_PA, _BOTH, dict(member=(3, 32), log_std=4098), -1,
     "fg_rollout_hd_actor_per_agent: member 3 differs from member 0 in hidden or out_tanh"),
    # NULL log_std: an error for the sampling entry; the deterministic actor elsewhere, whose logp_seq is then not looked at
    (("sample",), _BOTH, dict(log_std=None, B=0, logp=4098), -1, "fg_rollout_hd_actor_sample: log_std is NULL"),
    (("per_agent", "norm"), _RUN, dict(log_std=None, B=0, logp=4098), 0, None),
    (_GAUSS, _BOTH, dict(log_std=4098), -3, "fg_rollout_hd_actor_sample: log_std must be 4-byte aligned"),
    (("sample",), _RUN, dict(logp=4098), -3, "fg_rollout_hd_actor_sample: logp_seq must be 4-byte aligned"),
    (_PA, _RUN, dict(logp=4098), -3, "fg_rollout_hd_actor_per_agent: logp_seq must be 4-byte aligned"),
    (_LN, _RUN, dict(logp=4098), -3, "fg_rollout_hd_actor_norm: logp_seq must be 4-byte aligned"),
    (_GAUSS, _RUN, dict(log_std=4098, logp=4098), -3, "fg_rollout_hd_actor_sample: log_std must be 4-byte aligned"),
    # an empty batch: nothing to launch, but nothing to describe either - after the call's own checks
    (_ALL, _RUN, dict(B=0), 0, None),
    (_ALL, _DRY, dict(B=0), -1, "fg_describe_actor_launch: B > 0 required"),
    (_ONE, _DRY, dict(B=0, N=81), -2, "fg_rollout_hd_actor: " + _N_LIST),
    (_PA, _DRY, dict(B=0, N=81), -2, "fg_rollout_hd_actor_per_agent: " + _N_LIST),
    # the describe twins look at their out buffer first, each in its own name
    (("shared",), _DRY, dict(out=None, actor=None), -1, "fg_describe_actor_launch: out buffer required"),
    (("sample",), _DRY, dict(out=None, actor=None), -1, "fg_describe_actor_sample_launch: out buffer required"),
    (_PA, _DRY, dict(out=None, actor=None), -1, "fg_describe_actor_per_agent_launch: out buffer required"),
    (_LN, _DRY, dict(out=None, actor=None), -1, "fg_describe_actor_norm_launch: out buffer required"),
]


def _hd_actor_call(lib, kind, dry, H=64, N=9, K=20, B=128, actor="fake", member=None, norm="fake", log_std=4096, logp=4096,
                   out="buffer"):
    """(status, fg_last_error()) of the `kind` entry (its describe twin when `dry`) on stand-in pointers.  `member`:
    (index, hidden) of one per-agent member to alter; `norm`: None, or _fake_norm's keyword arguments."""
    if actor == "fake":
        actor = fake_actors(9, H) if kind == "per_agent" else _fake_actor(H)
        if member is not None:
            actor[member[0]].hidden = member[1]
    norm = _fake_norm() if norm == "fake" else norm if norm is None else _fake_norm(**norm)
    lead = {"shared": (actor,), "sample": (actor, log_std), "per_agent": (actor, log_std), "norm": (actor, norm, log_std)}[kind]
    if dry:
        buf = ctypes.create_string_buffer(512) if out == "buffer" else None
        rc = getattr(lib, HD_ACTOR_ENTRIES[kind][1])(_params(), *lead, B, N, K, 1, buf, 512)
    else:
        state = [ctypes.c_void_p(4096)] * 12 + ([] if kind == "shared" else [logp])
        rc = getattr(lib, HD_ACTOR_ENTRIES[kind][0])(_params(), *lead, B, N, K, *state, 1, None)
    return rc, lib.fg_last_error().decode()


def test_hd_actor_entries_fail_in_one_order_with_one_text():
    lib = _native.load()
    for kinds, dries, wrong, status, text in HD_ACTOR_BAD_CALLS:
        assert status != 0 or wrong.get("B") == 0, "a call that would launch: %r" % (wrong,)
        for kind in kinds:
            for dry in dries:
                rc, got = _hd_actor_call(lib, kind, dry, **wrong)
                assert rc == status and (text is None or got == text), (kind, dry, wrong, rc, got)


def test_log_prob_entry_checks_its_arguments_without_a_device():
    lib = _native.load()
    a = ctypes.c_void_p(4096)
    assert lib.fg_actor_log_prob(None, None, 0, None, None) == 0                    # no draws: a no-op
    assert lib.fg_actor_log_prob(a, a, -1, a, None) == -1
    assert lib.fg_actor_log_prob(None, a, 8, a, None) == -1 and lib.fg_actor_log_prob(a, None, 8, a, None) == -1
    assert lib.fg_actor_log_prob(a, a, 8, None, None) == -1
    assert lib.fg_actor_log_prob(ctypes.c_void_p(4100), a, 8, a, None) == -3       # eps: float2 units
    assert lib.fg_actor_log_prob(a, ctypes.c_void_p(4098), 8, a, None) == -3
    assert lib.fg_actor_log_prob(a, a, 8, ctypes.c_void_p(4098), None) == -3


def test_layernorm_kernels_use_no_scratch_and_the_others_keep_their_counts():
    from tests.isa_scan import kernel_resources
    ks = kernel_resources(LIB)
    for kern in ("ln_actor_kernel<", "ln_sample_kernel<"):
        mine = [k for k in ks if kern in k["demangled"]]
        assert len(mine) == len(FUSED_N) * len(FUSED_LN_HIDDEN) == 16, kern
        assert len({k["demangled"] for k in mine}) == len(mine)
        for k in mine:
            assert k["private_segment"] == 0 and k["vgpr_spill"] == 0, k
    nh = len(FUSED_N) * len(FUSED_HIDDEN)
    for kern, count in (("actor_rollout_kernel<", nh), ("actor_sample_kernel<", nh), ("pa_actor_kernel<", nh),
                        ("pa_sample_kernel<", nh), ("scn_lane_actor<", 14), ("scn_lane_actor_gauss<", 14)):
        assert len([k for k in ks if kern in k["demangled"]]) == count, kern
    assert len([k for k in ks if "scn_lane_actor" in k["demangled"]]) == 28
