"""CPU checks of the recurrent actor rollout (`fg_rollout_hd_actor_gru`, gru_actor_kernel / gru_sample_kernel): what
`RecurrentActor.forward` computes, which path a recurrent actor takes, what `resolve_actor` hands to the launch, the ctypes
mirror of FgActorGru, the dry-run description, the argument checks that touch no device, and the new kernels' resources."""
import copy
import ctypes
import os
import subprocess
import types

import pytest
import torch

from formation_gym import GaussianActor, PerAgentActor, RecurrentActor, _native, load_scenario
from formation_gym.actor_rollout import (FUSED_GRU_HIDDEN, FUSED_LN_HIDDEN, FUSED_N, ActorGru, FusedActor, actor_path,
                                         recurrent_mean, resolve_actor)
from tests.actor_testlib import LIB, ROOT, describe, fake_actor as _fake_actor, params as _params

nn = torch.nn


def _base(N, H, in_norm=True, norms=True, D=None):
    D = 6 * N if D is None else D
    mods = [nn.LayerNorm(D)] if in_norm else []
    mods += [nn.Linear(D, H), nn.ReLU()] + ([nn.LayerNorm(H)] if norms else [])
    mods += [nn.Linear(H, H), nn.ReLU()] + ([nn.LayerNorm(H)] if norms else [])
    return nn.Sequential(*mods)


def _actor(N, H, in_norm=True, tanh=False, cell=True, D=None):
    head = nn.Sequential(nn.Linear(H, 2), nn.Tanh()) if tanh else nn.Linear(H, 2)
    return RecurrentActor(_base(N, H, in_norm, D=D), nn.GRUCell(H, H) if cell else nn.GRU(H, H), nn.LayerNorm(H), head)


def test_fused_gru_hidden_is_its_own_constant():
    assert tuple(FUSED_GRU_HIDDEN) == (32, 64) and tuple(FUSED_GRU_HIDDEN) == tuple(FUSED_LN_HIDDEN)


@pytest.mark.parametrize("cell", [True, False])
def test_forward_is_the_formula(cell):
    torch.manual_seed(5)
    N, H = 4, 32
    actor = _actor(N, H, tanh=True, cell=cell).double()
    with torch.no_grad():
        for p in actor.parameters():
            p.add_(0.3 * torch.randn_like(p))
    obs, h = torch.randn(7, N, 6 * N, dtype=torch.float64), torch.rand(7, N, H, dtype=torch.float64) * 2 - 1
    with torch.no_grad():
        act, h1 = actor(obs, h)
        w_ih, w_hh, b_ih, b_hh = actor.gru_parameters()
        x = actor.base(obs)
        gi, gh = x @ w_ih.T + b_ih, h @ w_hh.T + b_hh
        r = torch.sigmoid(gi[..., :H] + gh[..., :H])
        z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
        n = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
        want_h = (1 - z) * n + z * h
        y = (want_h - want_h.mean(-1, keepdim=True)) / torch.sqrt(want_h.var(-1, unbiased=False, keepdim=True) + actor.norm.eps)
        y = y * actor.norm.weight + actor.norm.bias
        want_a = torch.tanh(y @ actor.head[0].weight.T + actor.head[0].bias)
    assert act.shape == (7, N, 2) and h1.shape == (7, N, H)
    assert float((h1 - want_h).abs().max()) <= 1e-12 and float((act - want_a).abs().max()) <= 1e-12
    # the state carried on is h', before the norm
    assert float((h1 - want_h).abs().max()) < float((h1 - y).abs().max())


def test_grucell_and_gru_members_agree():
    torch.manual_seed(6)
    N, H = 9, 64
    a = _actor(N, H, cell=True)
    b = copy.deepcopy(a)
    b.rnn = nn.GRU(H, H)
    with torch.no_grad():
        for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
            getattr(b.rnn, name + "_l0").copy_(getattr(a.rnn, name))
    obs, h = torch.randn(11, N, 6 * N), torch.rand(11, N, H) * 2 - 1
    with torch.no_grad():
        act_a, h_a = a(obs, h)
        act_b, h_b = b(obs, h)
        want = a.rnn(a.base(obs).reshape(-1, H), h.reshape(-1, H)).reshape(11, N, H)     # the module's own step
    assert torch.equal(act_a, act_b) and torch.equal(h_a, h_b) and torch.equal(h_a, want)
    # both as a Gaussian mean, and the state the helpers make
    g = GaussianActor(a)
    with torch.no_grad():
        act, h_g = g(obs, h)
        assert act.shape == (11, N, 2) and torch.equal(h_g, h_a)
        lp = g.log_prob(obs, act_a, h)
        assert torch.allclose(lp, torch.full_like(lp, -float(g.log_std.sum()) - 1.8378770664093453))
        assert torch.equal(g.distribution(obs, h).mean, act_a)
    h0 = a.initial_state(5, N)
    assert h0.shape == (5, N, H) and h0.dtype == torch.float32 and not bool(h0.any()) and h0.device == a.rnn.weight_ih.device
    assert recurrent_mean(a) is a and recurrent_mean(g) is a and recurrent_mean(a.base) is None


@pytest.mark.parametrize("H", FUSED_GRU_HIDDEN)
def test_recurrent_actor_fuses(H):
    for N in FUSED_N:
        for in_norm in (True, False):
            for tanh in (True, False):
                for cell in (True, False):
                    actor = _actor(N, H, in_norm, tanh, cell)
                    assert actor_path(actor, N) == "fused", (N, in_norm, tanh, cell)
                    assert actor_path(GaussianActor(actor), N) == "fused", (N, in_norm, tanh, cell)
    assert actor_path(RecurrentActor(_base(9, H), nn.GRU(H, H, batch_first=True), nn.LayerNorm(H), nn.Linear(H, 2)), 9) == "fused"


def test_recurrent_actor_host_paced():
    N, H = 9, 64
    good = _actor(N, H)
    assert actor_path(good, N) == "fused"
    no_norms = _actor(N, H)
    no_norms.base = _base(N, H, in_norm=False, norms=False)                        # a base without norms
    assert actor_path(no_norms, N) == "host" and actor_path(GaussianActor(no_norms), N) == "host"
    assert actor_path(_actor(N, 128), N) == "host"                                 # H = 128
    assert actor_path(_actor(N, 48), N) == "host"
    two = _actor(N, H)
    two.rnn = nn.GRU(H, H, num_layers=2)                                           # a multi-layer GRU
    assert actor_path(two, N) == "host"
    bi = _actor(N, H)
    bi.rnn = nn.GRU(H, H, bidirectional=True)                                      # a bidirectional GRU
    assert actor_path(bi, N) == "host"
    bare = _actor(N, H)
    bare.norm = None                                                               # no norm after the GRU
    assert actor_path(bare, N) == "host"
    ident = _actor(N, H)
    ident.norm = nn.Identity()
    assert actor_path(ident, N) == "host"
    members = PerAgentActor([_actor(N, H) for _ in range(N)])                      # recurrent PerAgentActor members
    assert actor_path(members, N) == "host" and actor_path(GaussianActor(members), N) == "host"
    # the GRU's own conditions
    nobias = _actor(N, H)
    nobias.rnn = nn.GRUCell(H, H, bias=False)
    assert actor_path(nobias, N) == "host"
    narrow = _actor(N, H)
    narrow.rnn = nn.GRUCell(H, 32)
    assert actor_path(narrow, N) == "host"
    lstm = _actor(N, H)
    lstm.rnn = nn.LSTMCell(H, H)
    assert actor_path(lstm, N) == "host"
    f64 = _actor(N, H)
    f64.rnn = nn.GRUCell(H, H).double()
    assert actor_path(f64, N) == "host"
    strided = _actor(N, H)
    strided.rnn.bias_hh = nn.Parameter(torch.zeros(6 * H)[::2])
    assert not strided.rnn.bias_hh.is_contiguous() and actor_path(strided, N) == "host"
    bad_eps = _actor(N, H)
    bad_eps.norm.eps = 0.0
    assert actor_path(bad_eps, N) == "host"
    wide_norm = _actor(N, H)
    wide_norm.norm = nn.LayerNorm(2 * H)
    assert actor_path(wide_norm, N) == "host"
    # the head's
    head3 = _actor(N, H)
    head3.head = nn.Linear(H, 3)
    assert actor_path(head3, N) == "host"
    relu_head = _actor(N, H)
    relu_head.head = nn.Sequential(nn.Linear(H, 2), nn.ReLU())
    assert actor_path(relu_head, N) == "host"
    # the base with its last Linear left in
    whole = _actor(N, H)
    whole.base = nn.Sequential(*_base(N, H), nn.Linear(H, H))
    assert actor_path(whole, N) == "host"
    # the env's facts, as for the other forms
    assert actor_path(good, N, device="cuda:0") == "host"                          # parameters off the env's device
    assert actor_path(good, 81) == "host" and actor_path(_actor(10, H), 10) == "host"
    for g in (good, GaussianActor(good)):
        assert actor_path(g, N, world_options=True) == "host" and actor_path(g, N, callback=True) == "host"
        assert actor_path(g, N, silent=False) == "host" and actor_path(g, N, continuous=False) == "host"
        assert actor_path(g, N, fused_scenario=False) == "host"
        assert actor_path(g, N, fused_gru_hidden=()) == "host" and actor_path(g, N, fused_gru_hidden=(32,)) == "host"
        assert actor_path(g, N, fused_ln_hidden=()) == "fused"                     # its own fact, not the LayerNorm actor's


def test_resolve_hands_back_the_modules_own_tensors():
    N, H = 9, 64
    for cell in (True, False):
        actor = _actor(N, H, tanh=True, cell=cell)
        actor.norm.eps = 3e-4
        fa = resolve_actor(actor, N)
        assert isinstance(fa, FusedActor) and (fa.hidden, fa.out_tanh, fa.per_agent, fa.log_std) == (H, True, False, None)
        b = actor.base
        for got, want in zip(fa.members[0], (b[1].weight, b[1].bias, b[4].weight, b[4].bias, actor.head[0].weight,
                                             actor.head[0].bias)):
            assert got is want
        assert len(fa.members) == 1
        assert fa.norms.input[0] is b[0].weight and fa.norms.hidden1[1] is b[3].bias and fa.norms.hidden2[0] is b[6].weight
        sfx = "" if cell else "_l0"
        assert isinstance(fa.gru, ActorGru)
        for got, name in zip(fa.gru[:4], ("weight_ih", "weight_hh", "bias_ih", "bias_hh")):
            assert got is getattr(actor.rnn, name + sfx)
        assert fa.gru.norm[0] is actor.norm.weight and fa.gru.norm[1] is actor.norm.bias and fa.gru.norm[2] == 3e-4
        s = _native.actor_gru(fa.gru)
        assert s.w_ih == actor.rnn.__getattr__("weight_ih" + sfx).data_ptr() and s.b_hh == fa.gru.b_hh.data_ptr()
        assert s.norm_gamma == actor.norm.weight.data_ptr() and s.norm_beta == actor.norm.bias.data_ptr()
        assert abs(s.norm_eps - 3e-4) < 1e-10
        g = GaussianActor(actor)
        fg = resolve_actor(g, N)
        assert fg.log_std is g.log_std and fg.gru.w_hh is fa.gru.w_hh and fg.members[0][4] is actor.head[0].weight
    plain_norm = _actor(N, H, in_norm=False)
    plain_norm.norm = nn.LayerNorm(H, elementwise_affine=False)
    fb = resolve_actor(plain_norm, N)
    assert fb.norms.input is None and fb.gru.norm[:2] == (None, None) and not fb.out_tanh
    s = _native.actor_gru(fb.gru)
    assert not s.norm_gamma and not s.norm_beta
    # the forms without a state keep gru = None
    ln = nn.Sequential(*_base(N, H), nn.Linear(H, 2))
    assert resolve_actor(ln, N).gru is None and resolve_actor(ln, N).norms is not None


@pytest.mark.parametrize("name,N,L,M,num_obs,D", [("basic_formation_env", 3, 3, 0, 0, 18),
                                                  ("formation_hd_partial_env", 5, 5, 0, 3, 26),
                                                  ("formation_hd_obs_env", 4, 4, 3, 0, 28)])
def test_landmark_scenarios_run_recurrent_actors_host_paced(name, N, L, M, num_obs, D):
    sc = load_scenario(name)
    world = types.SimpleNamespace(agents=[None] * N, landmarks=[None] * (L + M))
    sc.num_agents, sc.num_landmarks, sc.num_obstacles, sc.num_obs, sc.obs_range = N, L, M, num_obs, 0.0
    facts = sc.actor_fused_rule(world)
    assert facts["fused_gru_hidden"] == () and facts["fused_ln_hidden"] == ()
    for H in (32, 64):
        rec = _actor(N, H, D=D)
        assert actor_path(rec, N, fused_scenario=True, **facts) == "host"
        assert actor_path(GaussianActor(rec), N, fused_scenario=True, **facts) == "host"
        plain = nn.Sequential(nn.Linear(D, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 2))
        assert actor_path(plain, N, fused_scenario=True, **facts) == "fused"


# ---- the C ABI without a device ----


def _fake_norm(in_norm=1, eps=1e-5, **kw):
    addr = 4096
    d = dict(in_gamma=addr, in_beta=addr, h1_gamma=addr, h1_beta=addr, h2_gamma=addr, h2_beta=addr, in_eps=eps, h1_eps=eps,
             h2_eps=eps, in_norm=in_norm)
    d.update(kw)
    return _native.FgActorNorm(**d)


def _fake_gru(**kw):
    addr = 4096
    d = dict(w_ih=addr, w_hh=addr, b_ih=addr, b_hh=addr, norm_gamma=addr, norm_beta=addr, norm_eps=1e-5)
    d.update(kw)
    return _native.FgActorGru(**d)


def _describe(lib, N, H, sample, norm="default", gru="default", B=4096, K=20):
    norm = _fake_norm() if norm == "default" else norm
    gru = _fake_gru() if gru == "default" else gru
    return describe(lib, "fg_describe_actor_gru_launch", (_fake_actor(H), norm, gru, 4096 if sample else None), N, B, K)


def test_struct_layout_matches_the_header(tmp_path):
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "formation_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(FgActorGru));']
    for fname, _ in _native.FgActorGru._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(FgActorGru, %s));' % (fname, fname))
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(_native.FgActorGru)
    assert [f for f, _ in _native.FgActorGru._fields_] == ["w_ih", "w_hh", "b_ih", "b_hh", "norm_gamma", "norm_beta", "norm_eps"]
    for fname, _ in _native.FgActorGru._fields_:
        assert int(got[fname]) == getattr(_native.FgActorGru, fname).offset, fname
    assert _native.load().fg_abi_version() == 8                                    # an additive change


def test_describe_names_one_instantiation_per_shape():
    lib = _native.load()
    names = set()
    for N in FUSED_N:
        for H in FUSED_GRU_HIDDEN:
            for sample in (False, True):
                kernel = "gru_sample_kernel" if sample else "gru_actor_kernel"
                for in_norm in (1, 0):                                             # a run-time fact: the same instantiation
                    rc, text = _describe(lib, N, H, sample, _fake_norm(in_norm))
                    assert rc == 0, text
                    assert text.count(kernel + "<") == 1 and "%s<%d,%d>" % (kernel, N, H) in text, text
                    assert text.count("_kernel<") == 1, text
                    assert " grid " in text and " lds " in text
                    names.add(text.split(" ")[0])
                    lds = int(text.split(" lds ")[1].split(";")[0])
                    assert lds <= 160 * 1024
    assert len(names) == 2 * len(FUSED_N) * len(FUSED_GRU_HIDDEN)


_WHO = "fg_rollout_hd_actor_gru: "
# (what is wrong with the call, status, fg_last_error()); the checks before the recurrent layer's are fg_rollout_hd_actor_norm's,
# in their order, the norms' in this entry's name
BAD_CALLS = [
    (dict(K=0), -1, "fg_rollout_hd_actor: B >= 0 and K >= 1 required"),
    (dict(N=81), -2, "fg_rollout_hd_actor: N must be 3, 4, 8, 9, 16, 25, 27 or 32"),
    (dict(actor=None), -1, "fg_rollout_hd_actor: actor is NULL"),
    (dict(H=48), -1, "fg_rollout_hd_actor: hidden must be 32, 64 or 128"),
    (dict(norm=None), -1, _WHO + "norm is NULL"),
    (dict(H=128), -1, _WHO + "hidden must be 32 or 64 with LayerNorms"),
    (dict(H=128, gru=None), -1, _WHO + "hidden must be 32 or 64 with LayerNorms"),          # the norms before the GRU
    (dict(norm=dict(h2_eps=0.0)), -1, _WHO + "h2_eps must be positive and finite"),
    (dict(gru=None), -1, _WHO + "gru is NULL"),
    (dict(gru=dict(w_ih=None)), -1, _WHO + "w_ih is NULL"),
    (dict(gru=dict(w_hh=None)), -1, _WHO + "w_hh is NULL"),
    (dict(gru=dict(b_ih=None)), -1, _WHO + "b_ih is NULL"),
    (dict(gru=dict(b_hh=None)), -1, _WHO + "b_hh is NULL"),
    (dict(gru=dict(norm_eps=0.0)), -1, _WHO + "norm_eps must be positive and finite"),
    (dict(gru=dict(norm_eps=float("inf"))), -1, _WHO + "norm_eps must be positive and finite"),
    (dict(gru=dict(norm_eps=float("nan"))), -1, _WHO + "norm_eps must be positive and finite"),
    (dict(gru=dict(norm_eps=-1e-5)), -1, _WHO + "norm_eps must be positive and finite"),
    (dict(gru=dict(w_hh=4098)), -3, _WHO + "w_hh must be 4-byte aligned"),
    (dict(gru=dict(b_ih=4097)), -3, _WHO + "b_ih must be 4-byte aligned"),
    (dict(gru=dict(norm_beta=4098)), -3, _WHO + "norm_beta must be 4-byte aligned"),
    (dict(gru=dict(norm_eps=0.0, w_hh=4098)), -1, _WHO + "norm_eps must be positive and finite"),   # values before alignment
    (dict(gru=dict(w_hh=4098), log_std=4098), -3, _WHO + "w_hh must be 4-byte aligned"),            # the GRU before log_std
    (dict(log_std=4098), -3, "fg_rollout_hd_actor_sample: log_std must be 4-byte aligned"),
]
# the hidden state is the run entry's alone
BAD_STATE = [
    (dict(rnn_state=None), -1, _WHO + "rnn_state is NULL"),
    (dict(rnn_state=4104), -3, _WHO + "rnn_state must be 16-byte aligned"),
    (dict(rnn_state=None, gru=dict(norm_eps=0.0)), -1, _WHO + "rnn_state is NULL"),
    (dict(logp=4098), -3, _WHO + "logp_seq must be 4-byte aligned"),
]


def _call(lib, dry, H=64, N=9, K=20, B=128, actor="fake", norm="fake", gru="fake", log_std=4096, logp=4096, rnn_state=4096):
    actor = _fake_actor(H) if actor == "fake" else actor
    norm = _fake_norm() if norm == "fake" else norm if norm is None else _fake_norm(**norm)
    gru = _fake_gru() if gru == "fake" else gru if gru is None else _fake_gru(**gru)
    if dry:
        buf = ctypes.create_string_buffer(512)
        rc = lib.fg_describe_actor_gru_launch(_params(), actor, norm, gru, log_std, B, N, K, 1, buf, 512)
    else:
        rc = lib.fg_rollout_hd_actor_gru(_params(), actor, norm, gru, log_std, B, N, K, *([ctypes.c_void_p(4096)] * 12), logp,
                                         rnn_state, 1, None)
    return rc, lib.fg_last_error().decode()


def test_bad_arguments_rejected_without_a_device():
    lib = _native.load()
    for wrong, status, text in BAD_CALLS:
        for dry in (False, True):
            rc, got = _call(lib, dry, **wrong)
            assert rc == status and got == text, (dry, wrong, rc, got)
    for wrong, status, text in BAD_STATE:
        rc, got = _call(lib, False, **wrong)
        assert rc == status and got == text, (wrong, rc, got)
    # an empty batch: nothing to launch and no state needed, but nothing to describe either
    assert _call(lib, False, B=0, rnn_state=None)[0] == 0
    assert _call(lib, False, B=0, log_std=None, logp=4098)[0] == 0
    assert _call(lib, True, B=0) == (-1, "fg_describe_actor_launch: B > 0 required")
    assert lib.fg_describe_actor_gru_launch(_params(), None, None, None, None, 128, 9, 20, 1, None, 512) == -1
    assert lib.fg_last_error().decode() == "fg_describe_actor_gru_launch: out buffer required"


def test_recurrent_kernels_use_no_scratch():
    from tests.isa_scan import kernel_resources
    ks = kernel_resources(LIB)
    for kern in ("gru_actor_kernel<", "gru_sample_kernel<"):
        mine = [k for k in ks if kern in k["demangled"]]
        assert len(mine) == len(FUSED_N) * len(FUSED_GRU_HIDDEN) == 16, kern
        assert len({k["demangled"] for k in mine}) == len(mine)
        for k in mine:
            assert k["private_segment"] == 0 and k["vgpr_spill"] == 0, k
