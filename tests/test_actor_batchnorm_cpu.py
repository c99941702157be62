"""CPU checks of the BatchNorm actor rollout (`fg_rollout_hd_actor_bn`, `fg_rollout_hd_actor_bn_per_agent`; bn_actor_kernel,
bn_sample_kernel, pa_bn_actor_kernel, pa_bn_sample_kernel): `InputBatchNorm`, which path a BatchNorm actor takes and what
`resolve_actor` hands to the launch, the struct layout, the argument checks and dry runs that touch no device, the new kernels'
resources, and the error model of tests/actor_bn_testlib.py on CPU tensors - torch's fp32 modules inside the bound, every
mutant of the fp64 reference outside it."""
import copy
import ctypes
import os
import types

import pytest
import torch

import formation_gym
from formation_gym import GaussianActor, InputBatchNorm, PerAgentActor, RecurrentActor, _native, load_scenario
from formation_gym.actor_rollout import (FUSED_BN_HIDDEN, FUSED_HIDDEN, FUSED_N, ActorInBn, FusedActor, actor_path, actor_spec,
                                         batchnorm_spec, layernorm_spec, per_agent_bn_spec, per_agent_spec, resolve_actor,
                                         sample_spec)
from tests import actor_bn_testlib as bt
from tests.actor_testlib import LIB, ROOT, describe, fake_actor, fake_actors, params as _params

nn = torch.nn


def _bn_mlp(N, H, tanh=False, norm=InputBatchNorm, D=None, **kw):
    D = 6 * N if D is None else D
    mods = [norm(D, **kw), nn.Linear(D, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 2)]
    return nn.Sequential(*(mods + [nn.Tanh()] if tanh else mods)).eval()


def _plain_mlp(N, H, tanh=False):
    mods = [nn.Linear(6 * N, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 2)]
    return nn.Sequential(*(mods + [nn.Tanh()] if tanh else mods))


# ---- InputBatchNorm ----
@pytest.mark.parametrize("affine", [True, False])
def test_input_batchnorm_equals_batchnorm1d_on_the_flattened_rows(affine):
    torch.manual_seed(0)
    B, N, D = 5, 3, 18
    ours, ref = InputBatchNorm(D, eps=1e-3, momentum=0.3, affine=affine), nn.BatchNorm1d(D, eps=1e-3, momentum=0.3, affine=affine)
    assert isinstance(ours, nn.BatchNorm1d) and formation_gym.InputBatchNorm is InputBatchNorm
    with torch.no_grad():
        for m in (ours, ref):
            m.running_mean.copy_(torch.linspace(-1, 1, D))
            m.running_var.copy_(torch.linspace(0.5, 2, D))
            if affine:
                m.weight.copy_(torch.linspace(0.5, 1.5, D))
                m.bias.copy_(torch.linspace(-0.3, 0.3, D))
    x = torch.randn(B, N, D)
    with pytest.raises(RuntimeError):
        ref.eval()(x)                                                  # nn.BatchNorm1d takes axis 1 for the channels
    for mode in ("eval", "train", "train", "eval"):
        getattr(ours, mode)(); getattr(ref, mode)()
        got, want = ours(x), ref(x.reshape(-1, D)).reshape(B, N, D)
        assert got.shape == x.shape and torch.equal(got, want), mode
        assert torch.equal(ours.running_mean, ref.running_mean) and torch.equal(ours.running_var, ref.running_var), mode
        assert int(ours.num_batches_tracked) == int(ref.num_batches_tracked)
    assert torch.equal(ours.eval()(x[0]), ref.eval()(x[0]))            # 2-D rows: the same module
    with pytest.raises(ValueError):
        ours(torch.randn(B, N, D + 1))
    free = InputBatchNorm(D, track_running_stats=False)
    assert free.running_mean is None and free(x).shape == x.shape


def test_input_batchnorm_state_dict_round_trips_with_batchnorm1d():
    D = 24
    src = nn.BatchNorm1d(D)
    with torch.no_grad():
        src.running_mean.normal_(); src.running_var.uniform_(0.5, 2); src.weight.normal_(); src.bias.normal_()
        src.num_batches_tracked.fill_(17)
    ours = InputBatchNorm(D)
    assert set(ours.state_dict()) == set(src.state_dict())
    ours.load_state_dict(src.state_dict())
    back = nn.BatchNorm1d(D)
    back.load_state_dict(ours.state_dict())
    for k, v in src.state_dict().items():
        assert torch.equal(back.state_dict()[k], v) and torch.equal(ours.state_dict()[k], v), k


# ---- the path table ----
def test_fused_bn_hidden_is_its_own_constant():
    assert tuple(FUSED_BN_HIDDEN) == (32, 64) and set(FUSED_BN_HIDDEN) < set(FUSED_HIDDEN)
    import formation_gym.actor_rollout as ar
    assert "FUSED_BN_HIDDEN" in vars(ar) and "fused_bn_hidden" in ar._body_spec.__code__.co_varnames
    assert "fused_bn_hidden" in ar._recurrent_spec.__code__.co_varnames


@pytest.mark.parametrize("H", FUSED_BN_HIDDEN)
def test_batchnorm_actor_fuses(H):
    for N in FUSED_N:
        for tanh in (True, False):
            for norm in (InputBatchNorm, nn.BatchNorm1d):
                actor = _bn_mlp(N, H, tanh, norm)
                assert actor_path(actor, N) == "fused", (N, tanh, norm)
                assert actor_path(GaussianActor(actor), N) == "fused", (N, tanh, norm)
        pa = PerAgentActor([_bn_mlp(N, H, True, nn.BatchNorm1d) for _ in range(N)]).eval()
        assert actor_path(pa, N) == "fused" and actor_path(GaussianActor(pa), N) == "fused", N
    N = 9
    assert actor_path(_bn_mlp(N, H, affine=False), N) == "fused"
    assert actor_path(_bn_mlp(N, H, eps=3e-2), N) == "fused"
    mixed_affine = PerAgentActor([_bn_mlp(N, H, norm=nn.BatchNorm1d, affine=i % 2 == 0, eps=10.0 ** -(i % 4 + 1))
                                  for i in range(N)]).eval()
    assert actor_path(mixed_affine, N) == "fused"                      # each member its own eps and affine-ness


def test_resolve_hands_back_the_statistics_themselves():
    N, H = 9, 64
    actor = _bn_mlp(N, H, tanh=True, eps=2e-4)
    fa = resolve_actor(actor, N)
    assert isinstance(fa, FusedActor) and (fa.hidden, fa.out_tanh, fa.per_agent, fa.log_std, fa.norms, fa.gru) == \
        (H, True, False, None, None, None)
    for got, want in zip(fa.members[0], (actor[1].weight, actor[1].bias, actor[3].weight, actor[3].bias, actor[5].weight,
                                         actor[5].bias)):
        assert got is want
    bn = actor[0]
    assert isinstance(fa.in_bn, tuple) and len(fa.in_bn) == 5 and isinstance(fa.in_bn, ActorInBn)
    assert fa.in_bn[0] is bn.running_mean and fa.in_bn[1] is bn.running_var and fa.in_bn[2] is bn.weight
    assert fa.in_bn[3] is bn.bias and fa.in_bn[4] == 2e-4
    fb = resolve_actor(_bn_mlp(N, H, affine=False), N)
    assert fb.in_bn[2] is None and fb.in_bn[3] is None and not fb.out_tanh
    g = GaussianActor(actor)
    fg = resolve_actor(g, N)
    assert fg.log_std is g.log_std and fg.in_bn[0] is bn.running_mean
    pa = PerAgentActor([_bn_mlp(N, H, norm=nn.BatchNorm1d, eps=10.0 ** -(i + 1)) for i in range(N)]).eval()
    fp = resolve_actor(pa, N)
    assert fp.per_agent and len(fp.members) == N and isinstance(fp.in_bn, list) and len(fp.in_bn) == N
    for i, a in enumerate(pa.actors):
        assert fp.in_bn[i][0] is a[0].running_mean and fp.in_bn[i][4] == 10.0 ** -(i + 1) and fp.members[i][0] is a[1].weight
    # the ctypes struct the launch takes
    s = _native.actor_in_bn(fa.in_bn)
    assert s.mean == bn.running_mean.data_ptr() and s.var == bn.running_var.data_ptr() and s.gamma == bn.weight.data_ptr()
    assert s.beta == bn.bias.data_ptr() and abs(s.eps - 2e-4) < 1e-10
    s = _native.actor_in_bn(fb.in_bn)
    assert s.mean and s.var and not s.gamma and not s.beta
    # the specs: new functions for the new form, the old ones keep their shapes and never take it
    hidden, out_tanh, ws, in_bn = batchnorm_spec(actor, N)
    assert (hidden, out_tanh, len(ws)) == (H, True, 6) and in_bn[1] is bn.running_var
    hidden, out_tanh, wss, bns = per_agent_bn_spec(pa, N)
    assert (hidden, out_tanh, len(wss), len(bns)) == (H, False, N, N)
    assert actor_spec(actor, N) is None and layernorm_spec(actor, N) is None and per_agent_spec(pa, N) is None
    assert sample_spec(g, N) is None and batchnorm_spec(_plain_mlp(N, H), N) is None
    # existing positional constructions keep working, the new field defaults to None
    old = FusedActor(H, True, [[None] * 6], False, None)
    assert old.in_bn is None and old.norms is None and old.gru is None
    plain = resolve_actor(_plain_mlp(N, 128), N)
    assert plain.in_bn is None and plain.hidden == 128


def test_batchnorm_actor_host_paced():
    N, H = 9, 64
    good = _bn_mlp(N, H)
    assert actor_path(good, N) == "fused"
    good.train()
    assert actor_path(good, N) == "host" and actor_path(GaussianActor(good), N) == "host"      # batch statistics
    good.eval()
    assert actor_path(good, N) == "fused"                              # the rule is evaluated per call
    assert actor_path(_bn_mlp(N, H, track_running_stats=False), N) == "host"
    assert actor_path(_bn_mlp(N, 128), N) == "host" and actor_path(GaussianActor(_bn_mlp(N, 128)), N) == "host"
    assert actor_path(_bn_mlp(N, 48), N) == "host"
    later = nn.Sequential(nn.Linear(54, H), nn.BatchNorm1d(H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 2)).eval()
    assert actor_path(later, N) == "host"                              # a BatchNorm after the first Linear
    twice = nn.Sequential(InputBatchNorm(54), *_bn_mlp(N, H)).eval()
    assert actor_path(twice, N) == "host"
    ln = nn.Sequential(InputBatchNorm(54), nn.Linear(54, H), nn.ReLU(), nn.LayerNorm(H), nn.Linear(H, H), nn.ReLU(),
                       nn.LayerNorm(H), nn.Linear(H, 2)).eval()
    assert actor_path(ln, N) == "host"                                 # in front of the LayerNorm form
    ln2 = nn.Sequential(InputBatchNorm(54), nn.LayerNorm(54), *list(ln)[1:]).eval()
    assert actor_path(ln2, N) == "host"
    rec = RecurrentActor(nn.Sequential(*list(ln)[:7]), nn.GRUCell(H, H), nn.LayerNorm(H), nn.Linear(H, 2)).eval()
    assert actor_path(rec, N) == "host"                                # a BatchNorm base in a RecurrentActor
    rec_ok = RecurrentActor(nn.Sequential(*list(ln)[1:7]), nn.GRUCell(H, H), nn.LayerNorm(H), nn.Linear(H, 2))
    assert actor_path(rec_ok, N) == "fused"
    wrong = _bn_mlp(N, H)
    wrong[0] = InputBatchNorm(6 * N + 2).eval()
    assert actor_path(wrong, N) == "host"                              # num_features != D
    f64 = _bn_mlp(N, H)
    f64[0] = InputBatchNorm(6 * N).double().eval()
    assert actor_path(f64, N) == "host"                                # fp64 statistics
    f64s = _bn_mlp(N, H)
    f64s[0].running_var = f64s[0].running_var.double()
    assert actor_path(f64s, N) == "host"
    strided = _bn_mlp(N, H)
    strided[0].running_mean = torch.zeros(12 * N)[::2]
    assert actor_path(strided, N) == "host"
    bad_eps = _bn_mlp(N, H)
    bad_eps[0].eps = 0.0
    assert actor_path(bad_eps, N) == "host"

    class Sub(nn.BatchNorm1d):
        pass
    assert actor_path(_bn_mlp(N, H, norm=Sub), N) == "host"            # the module's type, not an instance check
    assert actor_path(good, N, device="cuda:0") == "host"              # parameters off the env's device
    assert actor_path(GaussianActor(good), N, device="cuda:0") == "host"
    assert actor_path(_bn_mlp(81, H), 81) == "host" and actor_path(_bn_mlp(10, H), 10) == "host"   # N outside FUSED_N
    # per-agent members: all or none, one H, one tanh flag, every one in eval mode
    members = [_bn_mlp(N, H, norm=nn.BatchNorm1d) for _ in range(N)]
    assert actor_path(PerAgentActor(members).eval(), N) == "fused"
    assert actor_path(PerAgentActor(members[:-1] + [_plain_mlp(N, H)]).eval(), N) == "host"          # mixed members
    assert actor_path(GaussianActor(PerAgentActor([_plain_mlp(N, H)] + members[1:]).eval()), N) == "host"
    assert actor_path(PerAgentActor(members[:-1] + [_bn_mlp(N, 32, norm=nn.BatchNorm1d)]).eval(), N) == "host"
    assert actor_path(PerAgentActor(members[:-1] + [_bn_mlp(N, H, True, nn.BatchNorm1d)]).eval(), N) == "host"
    pa = PerAgentActor(members).eval()
    pa.actors[4].train()
    assert actor_path(pa, N) == "host"
    assert actor_path(PerAgentActor([_bn_mlp(N, 128, norm=nn.BatchNorm1d) for _ in range(N)]).eval(), N) == "host"
    pa.eval()
    # the env's facts
    for g in (good, GaussianActor(good), pa):
        assert actor_path(g, N) == "fused"
        assert actor_path(g, N, world_options=True) == "host"
        assert actor_path(g, N, callback=True) == "host"
        assert actor_path(g, N, silent=False) == "host"
        assert actor_path(g, N, continuous=False) == "host"
        assert actor_path(g, N, fused_scenario=False) == "host"
        assert actor_path(g, N, fused_bn_hidden=()) == "host"
    assert actor_path(pa, N, per_agent=False) == "host"
    assert actor_path(_plain_mlp(N, H), N, fused_bn_hidden=()) == "fused"
    assert actor_path(good, N, fused_bn_hidden=(64,)) == "fused" and actor_path(good, N, fused_bn_hidden=(32,)) == "host"


@pytest.mark.parametrize("name,N,L,M,num_obs,D", [("basic_formation_env", 3, 3, 0, 0, 18),
                                                  ("formation_hd_partial_env", 5, 5, 0, 3, 26),
                                                  ("formation_hd_obs_env", 4, 4, 3, 0, 28)])
def test_landmark_scenarios_run_batchnorm_actors_host_paced(name, N, L, M, num_obs, D):
    sc = load_scenario(name)
    world = types.SimpleNamespace(agents=[None] * N, landmarks=[None] * (L + M))
    sc.num_agents, sc.num_landmarks, sc.num_obstacles, sc.num_obs, sc.obs_range = N, L, M, num_obs, 0.0
    facts = sc.actor_fused_rule(world)
    assert facts["fused_bn_hidden"] == ()
    assert facts["fused_ln_hidden"] == () and facts["fused_gru_hidden"] == () and facts["per_agent"] is False
    assert facts["in_features"] == D and facts["fused_n"] == (N,) and facts["fused_hidden"] == (32, 64)
    for H in (32, 64):
        bn = _bn_mlp(N, H, D=D)
        assert actor_path(bn, N, fused_scenario=True, **facts) == "host"
        assert actor_path(GaussianActor(bn), N, fused_scenario=True, **facts) == "host"
        plain = nn.Sequential(nn.Linear(D, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 2))
        assert actor_path(plain, N, fused_scenario=True, **facts) == "fused"       # the plain body still fuses there


# ---- the C ABI without a device ----
ENTRIES = ("fg_rollout_hd_actor_bn", "fg_rollout_hd_actor_bn_per_agent", "fg_describe_actor_bn_launch",
           "fg_describe_actor_bn_per_agent_launch")


def _fake_bn(**kw):
    d = dict(mean=4096, var=4096, gamma=4096, beta=4096, eps=1e-5)
    d.update(kw)
    return _native.FgActorInBn(**d)


def _fake_bns(N, **kw):
    return (_native.FgActorInBn * N)(*[_fake_bn(**kw) for _ in range(N)])


def test_struct_layout_matches_the_header(tmp_path):
    import subprocess
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "formation_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(FgActorInBn));']
    for fname, _ in _native.FgActorInBn._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(FgActorInBn, %s));' % (fname, fname))
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(_native.FgActorInBn)
    for fname, _ in _native.FgActorInBn._fields_:
        assert int(got[fname]) == getattr(_native.FgActorInBn, fname).offset, fname
    assert _native.load().fg_abi_version() == 8                                    # an additive change


def test_the_four_entries_are_exported():
    lib = ctypes.CDLL(LIB)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _native.SIGNATURES, name


def _call(lib, per_agent, dry, N=9, K=20, B=128, H=64, bn="fake", log_std=4096, logp=4096, member=None):
    """(status, fg_last_error()) of the shared or per-agent entry (its describe twin when `dry`) on stand-in pointers; `bn`:
    None, or _fake_bn's keyword arguments; `member`: the per-agent member they apply to (None: every one)."""
    M = max(N, 32)
    kw = {} if bn in ("fake", None) else bn
    if per_agent:
        actor = fake_actors(M, H)
        bns = None if bn is None else _fake_bns(M)
        if bn is not None and kw:
            for i in (range(M) if member is None else [member]):
                bns[i] = _fake_bn(**kw)
    else:
        actor, bns = fake_actor(H), None if bn is None else _fake_bn(**kw)
    lead = (actor, bns, log_std)
    if dry:
        buf = ctypes.create_string_buffer(512)
        name = "fg_describe_actor_bn_per_agent_launch" if per_agent else "fg_describe_actor_bn_launch"
        rc = getattr(lib, name)(_params(), *lead, B, N, K, 1, buf, 512)
    else:
        name = "fg_rollout_hd_actor_bn_per_agent" if per_agent else "fg_rollout_hd_actor_bn"
        rc = getattr(lib, name)(_params(), *lead, B, N, K, *([ctypes.c_void_p(4096)] * 12), logp, 1, None)
    return rc, lib.fg_last_error().decode()


_N_LIST = "N must be 3, 4, 8, 9, 16, 25, 27 or 32"
# (what is wrong, status, the shared entry's text, the per-agent entry's text); the stand-in member for the per-agent entry is 5
BAD_CALLS = [
    (dict(bn=None), -1, "fg_rollout_hd_actor_bn: in_bn is NULL", "fg_rollout_hd_actor_bn_per_agent: in_bn is NULL"),
    (dict(bn=dict(mean=None)), -1, "fg_rollout_hd_actor_bn: in_bn mean is NULL",
     "fg_rollout_hd_actor_bn_per_agent: member 5: in_bn mean is NULL"),
    (dict(bn=dict(var=None)), -1, "fg_rollout_hd_actor_bn: in_bn var is NULL",
     "fg_rollout_hd_actor_bn_per_agent: member 5: in_bn var is NULL"),
    (dict(bn=dict(eps=0.0)), -1, "fg_rollout_hd_actor_bn: in_bn eps must be positive and finite",
     "fg_rollout_hd_actor_bn_per_agent: member 5: in_bn eps must be positive and finite"),
    (dict(bn=dict(eps=-1e-5)), -1, "fg_rollout_hd_actor_bn: in_bn eps must be positive and finite",
     "fg_rollout_hd_actor_bn_per_agent: member 5: in_bn eps must be positive and finite"),
    (dict(bn=dict(eps=float("inf"))), -1, "fg_rollout_hd_actor_bn: in_bn eps must be positive and finite",
     "fg_rollout_hd_actor_bn_per_agent: member 5: in_bn eps must be positive and finite"),
    (dict(bn=dict(eps=float("nan"))), -1, "fg_rollout_hd_actor_bn: in_bn eps must be positive and finite",
     "fg_rollout_hd_actor_bn_per_agent: member 5: in_bn eps must be positive and finite"),
    (dict(bn=dict(mean=4098)), -3, "fg_rollout_hd_actor_bn: in_bn mean must be 4-byte aligned",
     "fg_rollout_hd_actor_bn_per_agent: member 5: in_bn mean must be 4-byte aligned"),
    (dict(bn=dict(var=4097)), -3, "fg_rollout_hd_actor_bn: in_bn var must be 4-byte aligned",
     "fg_rollout_hd_actor_bn_per_agent: member 5: in_bn var must be 4-byte aligned"),
    (dict(bn=dict(gamma=4098)), -3, "fg_rollout_hd_actor_bn: in_bn gamma must be 4-byte aligned",
     "fg_rollout_hd_actor_bn_per_agent: member 5: in_bn gamma must be 4-byte aligned"),
    (dict(bn=dict(beta=4099)), -3, "fg_rollout_hd_actor_bn: in_bn beta must be 4-byte aligned",
     "fg_rollout_hd_actor_bn_per_agent: member 5: in_bn beta must be 4-byte aligned"),
    (dict(bn=dict(eps=0.0, beta=4099)), -1, "fg_rollout_hd_actor_bn: in_bn eps must be positive and finite",
     "fg_rollout_hd_actor_bn_per_agent: member 5: in_bn eps must be positive and finite"),
    # what fg_rollout_hd_actor_sample and fg_rollout_hd_actor_per_agent check, with their texts and in their order
    (dict(H=48), -1, "fg_rollout_hd_actor: hidden must be 32, 64 or 128", "fg_rollout_hd_actor: hidden must be 32, 64 or 128"),
    (dict(N=81), -2, "fg_rollout_hd_actor: " + _N_LIST, "fg_rollout_hd_actor_per_agent: " + _N_LIST),
    (dict(K=0), -1, "fg_rollout_hd_actor: B >= 0 and K >= 1 required", "fg_rollout_hd_actor_per_agent: B >= 0 and K >= 1 required"),
    (dict(B=-1), -1, "fg_rollout_hd_actor: B >= 0 and K >= 1 required", "fg_rollout_hd_actor_per_agent: B >= 0 and K >= 1 required"),
    (dict(N=81, bn=None), -2, "fg_rollout_hd_actor: " + _N_LIST, "fg_rollout_hd_actor_per_agent: " + _N_LIST),
    (dict(bn=None, log_std=4098), -1, "fg_rollout_hd_actor_bn: in_bn is NULL", "fg_rollout_hd_actor_bn_per_agent: in_bn is NULL"),
    (dict(log_std=4098), -3, "fg_rollout_hd_actor_sample: log_std must be 4-byte aligned",
     "fg_rollout_hd_actor_sample: log_std must be 4-byte aligned"),
]


def test_bad_arguments_rejected_without_a_device():
    lib = _native.load()
    for wrong, status, shared_text, pa_text in BAD_CALLS:
        for dry in (False, True):
            rc, got = _call(lib, False, dry, **wrong)
            assert (rc, got) == (status, shared_text), (wrong, dry, rc, got)
            rc, got = _call(lib, True, dry, member=5, **wrong)
            assert (rc, got) == (status, pa_text), (wrong, dry, rc, got)
    # hidden = 128: FG_ERR_BAD_ARG naming the field (and, per agent, the first member)
    for dry in (False, True):
        rc, got = _call(lib, False, dry, H=128)
        assert rc == -1 and got == "fg_rollout_hd_actor_bn: hidden must be 32 or 64 with an input BatchNorm", got
        rc, got = _call(lib, True, dry, H=128)
        assert rc == -1 and got == "fg_rollout_hd_actor_bn_per_agent: member 0: hidden must be 32 or 64 with an input BatchNorm"
    # the last member's index; members past N are not looked at
    rc, got = _call(lib, True, False, N=9, bn=dict(var=None), member=8)
    assert rc == -1 and "member 8: in_bn var is NULL" in got
    assert _call(lib, True, False, N=9, B=0, bn=dict(var=None), member=9)[0] == 0
    # logp_seq: 4-byte aligned with a log_std, ignored without one; an empty batch is a no-op, but there is nothing to describe
    rc, got = _call(lib, False, False, logp=4098)
    assert rc == -3 and got == "fg_rollout_hd_actor_bn: logp_seq must be 4-byte aligned"
    rc, got = _call(lib, True, False, logp=4098)
    assert rc == -3 and got == "fg_rollout_hd_actor_bn_per_agent: logp_seq must be 4-byte aligned"
    for per_agent in (False, True):
        assert _call(lib, per_agent, False, B=0, log_std=None, logp=4098)[0] == 0
        assert _call(lib, per_agent, False, B=0)[0] == 0
        assert _call(lib, per_agent, True, B=0) == (-1, "fg_describe_actor_launch: B > 0 required")


def test_describe_names_one_instantiation_per_shape_with_the_plain_twins_geometry():
    lib = _native.load()
    names = set()
    for N in FUSED_N:
        for H in FUSED_BN_HIDDEN:
            for sample in (False, True):
                ls = 4096 if sample else None
                for per_agent in (False, True):
                    kernel = ("pa_bn_" if per_agent else "bn_") + ("sample_kernel" if sample else "actor_kernel")
                    if per_agent:
                        rc, text = describe(lib, "fg_describe_actor_bn_per_agent_launch", (fake_actors(N, H), _fake_bns(N), ls), N)
                        rc2, twin = describe(lib, "fg_describe_actor_per_agent_launch", (fake_actors(N, H), ls), N)
                    else:
                        rc, text = describe(lib, "fg_describe_actor_bn_launch", (fake_actor(H), _fake_bn(), ls), N)
                        rc2, twin = (describe(lib, "fg_describe_actor_sample_launch", (fake_actor(H), ls), N) if sample
                                     else describe(lib, "fg_describe_actor_launch", (fake_actor(H),), N))
                    assert rc == 0 and rc2 == 0, (text, twin)
                    assert text.startswith("%s<%d,%d> " % (kernel, N, H)) and text.count("_kernel<") == 1, text
                    geometry = lambda t: t.split("> ")[1].split(" lds ")[0]
                    assert geometry(text) == geometry(twin), (text, twin)          # grid, block, envs per workgroup
                    lds, twin_lds = (int(t.split(" lds ")[1].split(";")[0]) for t in (text, twin))
                    pad = (6 * N + 3) // 4 * 4
                    assert lds == twin_lds + (0 if per_agent else 16 * pad) and lds <= 160 * 1024, (text, twin)
                    names.add(text.split(" ")[0])
    assert len(names) == 4 * len(FUSED_N) * len(FUSED_BN_HIDDEN) == 64


def test_batchnorm_kernels_use_no_scratch_and_the_others_keep_their_counts():
    from tests.isa_scan import kernel_resources
    ks = kernel_resources(LIB)
    for kern in (" fg::bn_actor_kernel<", " fg::bn_sample_kernel<", "pa_bn_actor_kernel<", "pa_bn_sample_kernel<"):
        mine = [k for k in ks if kern in " " + k["demangled"]]
        assert len(mine) == len(FUSED_N) * len(FUSED_BN_HIDDEN) == 16, (kern, len(mine))
        assert len({k["demangled"] for k in mine}) == len(mine)
        for k in mine:
            assert k["private_segment"] == 0 and k["vgpr_spill"] == 0, k
    nh = len(FUSED_N) * len(FUSED_HIDDEN)
    for kern, count in (("actor_rollout_kernel<", nh), ("actor_sample_kernel<", nh), ("pa_actor_kernel<", nh),
                        ("pa_sample_kernel<", nh), ("ln_actor_kernel<", 16), ("ln_sample_kernel<", 16),
                        ("gru_actor_kernel<", 16), ("gru_sample_kernel<", 16)):
        assert len([k for k in ks if kern in k["demangled"]]) == count, kern


# ---- the error model ----
@pytest.mark.parametrize("N,H,tanh,eps,affine,small_var", [(3, 64, True, 1e-5, True, False), (9, 64, False, 1e-5, True, False),
                                                           (27, 32, False, 1e-5, False, False), (32, 64, True, 1e-2, True, True),
                                                           (25, 64, False, 1e-1, True, True)])
def test_error_model_holds_fp32_and_sees_every_mutant(N, H, tanh, eps, affine, small_var):
    actor = bt.bn_actor(N, H, tanh, seed=N, eps=eps, affine=affine, small_var=small_var)
    ref = copy.deepcopy(actor).double()
    x = bt.rows(N, 133 * 24)
    with torch.no_grad():
        a32, a64 = actor(x), ref(x.double())
        bound = bt.bn_bound(ref, a64)
        own = float(((a32.double() - a64).abs() / bound).max())
        assert own <= 1.0, own                                          # torch's fp32 modules: inside
        # the same figure through the GPU tests' helper, on [K, B, N, D] observations
        o = x[:24 * N].reshape(2, 12, N, 6 * N)
        assert bt.bn_fidelity(actor, list(o), actor(o)) <= 1.0
        for name in bt.MUTANTS:
            if (name == "gamma_ignored" or name == "beta_ignored") and not affine:
                continue
            if name == "eps_left_out" and not small_var:
                continue                                                # eps decides only where the variance is tiny
            ratio = float(((bt.mutant(ref, name, x.double()) - a64).abs() / bound).max())
            assert ratio >= 10.0, (name, ratio)


def test_per_agent_fidelity_helper_uses_each_members_own_reference():
    N, H = 4, 32
    pa = bt.per_agent_bn_actor(N, H, tanh=True, seed=3)
    assert [type(a[0]) for a in pa.actors] == [nn.BatchNorm1d] * N and actor_path(pa, N) == "fused"
    assert len({float(a[0].eps) for a in pa.actors}) == 3 and pa.actors[2][0].weight is None
    o = bt.rows(N, 24 * N).reshape(2, 12, N, 6 * N)
    with torch.no_grad():
        got = torch.stack([pa(ok) for ok in o])                          # plain BatchNorm1d members see 2-D rows
        assert bt.bn_fidelity(pa, list(o), got) <= 1.0
        swapped = PerAgentActor(list(pa.actors)[1:] + [pa.actors[0]]).eval()
        assert bt.bn_fidelity(swapped, list(o), got) >= 10.0            # members permuted: far outside
    same = bt.per_agent_bn_actor(N, H, seed=3, identical=True)
    for a in same.actors[1:]:
        for p, q in zip(a.state_dict().values(), same.actors[0].state_dict().values()):
            assert torch.equal(p, q)
