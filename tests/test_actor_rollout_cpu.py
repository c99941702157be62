"""CPU checks of the learned-actor rollout (`env.rollout_actor`, `fg_rollout_hd_actor`): which path an actor takes, the
dry-run description of the fused launch, argument checks that touch no device, and the new kernels' resources."""
import ctypes

import pytest
import torch

from formation_gym import _native
from formation_gym.actor_rollout import FUSED_HIDDEN, FUSED_N, actor_path, actor_spec
from tests.actor_testlib import LIB, describe, fake_actor as _fake_actor, params as _params


def _mlp(N, H, tanh, dtype=torch.float32):
    mods = [torch.nn.Linear(6 * N, H), torch.nn.ReLU(), torch.nn.Linear(H, H), torch.nn.ReLU(), torch.nn.Linear(H, 2)]
    if tanh:
        mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods).to(dtype)


@pytest.mark.parametrize("H", FUSED_HIDDEN)
@pytest.mark.parametrize("tanh", [True, False])
def test_fusable_actors(H, tanh):
    for N in (9, 27):
        actor = _mlp(N, H, tanh)
        assert actor_path(actor, N) == "fused"
        hidden, out_tanh, ws = actor_spec(actor, N)
        assert (hidden, out_tanh) == (H, tanh) and len(ws) == 6


def test_bias_free_actor_fuses():
    actor = torch.nn.Sequential(torch.nn.Linear(54, 64, bias=False), torch.nn.ReLU(), torch.nn.Linear(64, 64),
                                torch.nn.ReLU(), torch.nn.Linear(64, 2, bias=False))
    assert actor_path(actor, 9) == "fused"
    assert actor_spec(actor, 9)[2][1] is None


def test_host_paced_actors():
    N = 9
    H48 = _mlp(N, 48, True)
    gelu = torch.nn.Sequential(torch.nn.Linear(54, 64), torch.nn.GELU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                               torch.nn.Linear(64, 2))
    deep = torch.nn.Sequential(torch.nn.Linear(54, 64), torch.nn.ReLU(), torch.nn.Linear(64, 64), torch.nn.ReLU(),
                               torch.nn.Linear(64, 64), torch.nn.ReLU(), torch.nn.Linear(64, 2))
    f64 = _mlp(N, 64, True, dtype=torch.float64)
    per_agent = [_mlp(N, 64, True) for _ in range(N)]
    for actor in (H48, gelu, deep, f64, per_agent, lambda o: o[..., :2]):
        assert actor_path(actor, N) == "host"
    assert actor_path(_mlp(81, 64, True), 81) == "host"                     # N = 81: no fused instantiation
    assert actor_path(_mlp(N, 64, True), 10) == "host"                      # input width is not 6N
    good = _mlp(N, 64, True)
    assert actor_path(good, N) == "fused"
    assert actor_path(good, N, fused_scenario=False) == "host"              # another scenario
    assert actor_path(good, N, silent=False) == "host"                      # non-silent agents (communication)
    assert actor_path(good, N, continuous=False) == "host"
    assert actor_path(good, N, world_options=True) == "host"                # walls, per-agent props, noise ...
    assert actor_path(good, N, callback=True) == "host"                     # a post_step_callback
    assert actor_path(good, N, device="cuda:0") == "host"                   # parameters not on the env's device


def _describe(lib, N, H, B=4096, K=20):
    return describe(lib, "fg_describe_actor_launch", (_fake_actor(H),), N, B, K)


def test_describe_names_one_instantiation_per_shape():
    lib = _native.load()
    names = set()
    for N in FUSED_N:
        for H in FUSED_HIDDEN:
            rc, text = _describe(lib, N, H)
            assert rc == 0, text
            assert text.count("actor_rollout_kernel<") == 1 and "actor_rollout_kernel<%d,%d>" % (N, H) in text
            names.add(text.split(" ")[0])
    assert len(names) == len(FUSED_N) * len(FUSED_HIDDEN)


def test_bad_arguments_rejected_without_a_device():
    lib = _native.load()
    f = ctypes.c_void_p(4096)
    ptrs = [f] * 12

    def call(N=9, K=20, actor=None):
        return lib.fg_rollout_hd_actor(_params(), actor if actor is not None else _fake_actor(64), 128, N, K, *ptrs, 1, None)
    assert call(actor=_fake_actor(48)) == -1                                  # FG_ERR_BAD_ARG: hidden width
    assert b"hidden" in lib.fg_last_error()
    assert call(N=81) == -2                                                   # FG_ERR_UNSUPPORTED_N
    no_w1 = _fake_actor(64)
    no_w1.w1 = None
    assert call(actor=no_w1) == -1
    assert call(K=0) == -1
    rc, _ = _describe(lib, 81, 64)
    assert rc == -2


def test_actor_kernels_use_no_scratch():
    from tests.isa_scan import kernel_resources
    ks = [k for k in kernel_resources(LIB) if "actor_rollout_kernel<" in k["demangled"]]
    assert len(ks) == len(FUSED_N) * len(FUSED_HIDDEN)
    for k in ks:
        assert k["private_segment"] == 0 and k["vgpr_spill"] == 0, k
        # 256-thread workgroups: up to 512 registers per lane are addressable; the widest (H = 128) passes hold 2 x 8 x 4
        # accumulators plus the weight fragments in flight.  A build well above this bound has started to hoist weights.
        assert k["vgpr"] <= 320, k
