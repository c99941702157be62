"""CPU checks of per-agent actors (`PerAgentActor`, `fg_rollout_hd_actor_per_agent`): which path they take, `forward`, the
dry-run description of the fused launch, argument checks that touch no device, and the new kernels' resources."""
import ctypes

import pytest
import torch

from formation_gym import PerAgentActor, _native
from formation_gym.actor_rollout import FUSED_HIDDEN, FUSED_N, GaussianActor, actor_path, per_agent_spec
from tests.actor_testlib import LIB, describe, fake_actors as _fake_actors, params as _params


def _mlp(N, H, tanh, dtype=torch.float32):
    mods = [torch.nn.Linear(6 * N, H), torch.nn.ReLU(), torch.nn.Linear(H, H), torch.nn.ReLU(), torch.nn.Linear(H, 2)]
    if tanh:
        mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods).to(dtype)


def _pa(N, H, tanh):
    return PerAgentActor([_mlp(N, H, tanh) for _ in range(N)])


@pytest.mark.parametrize("H", FUSED_HIDDEN)
@pytest.mark.parametrize("tanh", [True, False])
def test_per_agent_actor_fuses_for_every_shape(H, tanh):
    for N in FUSED_N:
        pa = _pa(N, H, tanh)
        assert actor_path(pa, N) == "fused"
        assert actor_path(GaussianActor(pa), N) == "fused"
        hidden, out_tanh, members = per_agent_spec(pa, N)
        assert (hidden, out_tanh) == (H, tanh) and len(members) == N and all(len(ws) == 6 for ws in members)
        assert members[-1][0] is pa.actors[-1][0].weight


def test_resolve_actor_returns_one_record_for_every_kind():
    """The record `MultiAgentEnv.rollout_actor` hands to `bind_rollout_actor`: the members are the actors' own tensors, one
    entry for a shared actor and N for a PerAgentActor; the env's facts and the scenario's per_agent fact send it host-paced."""
    from formation_gym.actor_rollout import actor_spec, landmark_facts, resolve_actor
    N, H = 9, 64
    shared, pa = _mlp(N, H, True), _pa(N, H, False)
    r = resolve_actor(shared, N)
    assert (r.hidden, r.out_tanh, r.per_agent, r.log_std) == (H, True, False, None)
    assert len(r.members) == 1 and all(x is y for x, y in zip(r.members[0], actor_spec(shared, N)[2]))
    g = GaussianActor(shared)
    r = resolve_actor(g, N)
    assert r.log_std is g.log_std and not r.per_agent and r.members[0][0] is shared[0].weight
    r = resolve_actor(pa, N)
    assert (r.hidden, r.out_tanh, r.per_agent, r.log_std) == (H, False, True, None) and len(r.members) == N
    assert all(ws[0] is a[0].weight and len(ws) == 6 for ws, a in zip(r.members, pa.actors))
    g = GaussianActor(pa)
    r = resolve_actor(g, N)
    assert r.per_agent and r.log_std is g.log_std and len(r.members) == N
    with pytest.raises(AttributeError):
        r.hidden = 32                                     # immutable
    for actor in (shared, pa, g):
        assert resolve_actor(actor, N, callback=True) is None and actor_path(actor, N, callback=True) == "host"
        assert resolve_actor(actor, N, world_options=True) is None and resolve_actor(actor, N, silent=False) is None
    assert resolve_actor(pa, N, per_agent=False) is None and resolve_actor(shared, N, per_agent=False) is not None
    assert resolve_actor(_mlp(N, 48, True), N) is None and resolve_actor(lambda o: o, N) is None
    facts = landmark_facts(1, 3, 3, 0, 0, 18)
    assert resolve_actor(_mlp(3, 64, True), 3, **facts).hidden == 64 and resolve_actor(_pa(3, 64, True), 3, **facts) is None


def test_bias_free_member_fuses():
    N = 9
    pa = _pa(N, 64, True)
    pa.actors[4] = torch.nn.Sequential(torch.nn.Linear(54, 64, bias=False), torch.nn.ReLU(), torch.nn.Linear(64, 64),
                                       torch.nn.ReLU(), torch.nn.Linear(64, 2, bias=False), torch.nn.Tanh())
    assert actor_path(pa, N) == "fused"
    assert per_agent_spec(pa, N)[2][4][1] is None


def test_per_agent_host_paced():
    N = 9
    good = _pa(N, 64, True)
    assert actor_path(PerAgentActor([_mlp(N, 64, True) for _ in range(N - 1)]), N) == "host"     # member count
    mixed_h = _pa(N, 64, True)
    mixed_h.actors[5] = _mlp(N, 32, True)
    mixed_tanh = _pa(N, 64, True)
    mixed_tanh.actors[0] = _mlp(N, 64, False)
    unfusable = _pa(N, 64, True)
    unfusable.actors[2] = torch.nn.Sequential(torch.nn.Linear(54, 64), torch.nn.GELU(), torch.nn.Linear(64, 64),
                                              torch.nn.ReLU(), torch.nn.Linear(64, 2))
    f64 = _pa(N, 64, True)
    f64.actors[7] = _mlp(N, 64, True, dtype=torch.float64)
    for pa in (mixed_h, mixed_tanh, unfusable, f64):
        assert actor_path(pa, N) == "host"
        assert actor_path(GaussianActor(pa), N) == "host"
        assert per_agent_spec(pa, N) is None
    assert actor_path(good, N, device="cuda:0") == "host"                   # parameters not on the env's device
    assert actor_path(GaussianActor(good, torch.zeros(2, dtype=torch.float64)), N) == "host"   # log_std not fp32
    assert actor_path(good, N) == "fused"
    for kw in (dict(fused_scenario=False), dict(silent=False), dict(world_options=True), dict(callback=True),
               dict(continuous=False)):
        assert actor_path(good, N, **kw) == "host"
        assert actor_path(GaussianActor(good), N, **kw) == "host"


def test_existing_decisions_unchanged():
    N = 9
    assert actor_path(_mlp(N, 64, True), N) == "fused"
    assert actor_path(GaussianActor(_mlp(N, 64, True)), N) == "fused"
    assert actor_path([_mlp(N, 64, True) for _ in range(N)], N) == "host"          # a plain list stays host-paced
    assert actor_path(torch.nn.ModuleList([_mlp(N, 64, True) for _ in range(N)]), N) == "host"
    assert actor_path(lambda o: o[..., :2], N) == "host"
    assert per_agent_spec(_mlp(N, 64, True), N) is None


def test_forward_is_the_per_agent_loop():
    torch.manual_seed(0)
    N = 4
    pa = _pa(N, 32, True)
    obs = torch.randn(5, 3, N, 6 * N)
    ref = torch.stack([pa.actors[i](obs[..., i, :]) for i in range(N)], dim=-2)
    assert torch.equal(pa(obs), ref)
    assert pa(obs).shape == (5, 3, N, 2)
    with pytest.raises(ValueError):
        pa(obs[..., :3, :])


def _describe(lib, N, H, log_std=None, B=4096, K=20, actors=None):
    actors = actors if actors is not None else _fake_actors(N, H)
    return describe(lib, "fg_describe_actor_per_agent_launch", (actors, log_std), N, B, K)


@pytest.mark.parametrize("sample", [False, True])
def test_describe_names_one_instantiation_per_shape(sample):
    lib = _native.load()
    kern = "pa_sample_kernel" if sample else "pa_actor_kernel"
    names = set()
    for N in FUSED_N:
        for H in FUSED_HIDDEN:
            rc, text = _describe(lib, N, H, log_std=ctypes.c_void_p(4096) if sample else None)
            assert rc == 0, text
            assert text.count("_kernel<") == 1 and "%s<%d,%d>" % (kern, N, H) in text, text
            names.add(text.split(" ")[0])
    assert len(names) == len(FUSED_N) * len(FUSED_HIDDEN)


def test_bad_arguments_rejected_without_a_device():
    lib = _native.load()
    f = ctypes.c_void_p(4096)
    ptrs = [f] * 13

    def call(N=9, K=20, actors=None, log_std=None):
        return lib.fg_rollout_hd_actor_per_agent(_params(), actors if actors is not None else _fake_actors(N, 64), log_std,
                                                 128, N, K, *ptrs, 1, None)
    no_w1 = _fake_actors(9, 64)
    no_w1[6].w1 = None
    assert call(actors=no_w1) == -1                                            # FG_ERR_BAD_ARG: a NULL member weight
    mixed_h = _fake_actors(9, 64)
    mixed_h[3].hidden = 32
    assert call(actors=mixed_h) == -1
    assert b"member 3" in lib.fg_last_error()
    mixed_tanh = _fake_actors(9, 64)
    mixed_tanh[8].out_tanh = 0
    assert call(actors=mixed_tanh) == -1
    assert b"member 8" in lib.fg_last_error()
    bad_hidden = _fake_actors(9, 48)
    assert call(actors=bad_hidden) == -1
    misaligned = _fake_actors(9, 64)
    misaligned[2].w2 = 4098
    assert call(actors=misaligned) == -3                                       # FG_ERR_ALIGNMENT
    assert call(log_std=ctypes.c_void_p(4098)) == -3
    assert call(N=81, actors=_fake_actors(9, 64)) == -2                         # FG_ERR_UNSUPPORTED_N, before any member
    assert call(K=0) == -1
    assert lib.fg_rollout_hd_actor_per_agent(_params(), None, None, 128, 9, 20, *ptrs, 1, None) == -1
    assert _describe(lib, 81, 64, actors=_fake_actors(9, 64))[0] == -2
    assert _describe(lib, 9, 64, actors=mixed_h)[0] == -1
    assert _describe(lib, 9, 64, actors=misaligned)[0] == -3


def test_per_agent_kernels_use_no_scratch():
    from tests.isa_scan import kernarg_sizes, kernel_resources
    ks = kernel_resources(LIB)
    for kern in ("pa_actor_kernel<", "pa_sample_kernel<"):
        sel = [k for k in ks if kern in k["demangled"]]
        assert len(sel) == len(FUSED_N) * len(FUSED_HIDDEN), kern
        for k in sel:
            assert k["private_segment"] == 0 and k["vgpr_spill"] == 0, k
            assert k["vgpr"] <= 320, k                    # the bound of the shared actor kernels
    sizes = kernarg_sizes(LIB)
    pa = {n: s for n, s in sizes.items() if "pa_actor_kernel" in n or "pa_sample_kernel" in n}
    assert len(pa) == 2 * len(FUSED_N) * len(FUSED_HIDDEN)
    # the by-value table of 6 x 32 weight pointers rides in the kernel arguments: within HIP's 4 KiB kernel-argument limit
    assert all(1536 < s <= 4096 for s in pa.values()), pa

