"""CPU checks of the Gaussian actor rollout (`GaussianActor`, `fg_rollout_hd_actor_sample`, `fg_actor_noise`): which path a
GaussianActor takes, the dry-run description of the sampling launch, argument checks that touch no device, the sampling
kernels' resources, and the distribution methods against torch.distributions.Normal."""
import ctypes

import pytest
import torch

from formation_gym import GaussianActor, _native
from formation_gym.actor_rollout import FUSED_HIDDEN, FUSED_N, actor_path
from tests.actor_testlib import LIB, describe, fake_actor as _fake_actor, params as _params


def _mlp(N, H, tanh=False, dtype=torch.float32):
    mods = [torch.nn.Linear(6 * N, H), torch.nn.ReLU(), torch.nn.Linear(H, H), torch.nn.ReLU(), torch.nn.Linear(H, 2)]
    if tanh:
        mods.append(torch.nn.Tanh())
    return torch.nn.Sequential(*mods).to(dtype)


@pytest.mark.parametrize("H", FUSED_HIDDEN)
def test_gaussian_actor_fuses_for_every_shape(H):
    for N in FUSED_N:
        for tanh in (False, True):
            assert actor_path(GaussianActor(_mlp(N, H, tanh)), N) == "fused"


def test_gaussian_actor_host_paced():
    N = 9
    gelu = torch.nn.Sequential(torch.nn.Linear(54, 64), torch.nn.GELU(), torch.nn.Linear(64, 2))
    assert actor_path(GaussianActor(gelu), N) == "host"                           # a mean that cannot fuse
    assert actor_path(GaussianActor(_mlp(N, 48)), N) == "host"
    g = GaussianActor(_mlp(N, 64))
    assert actor_path(g, N) == "fused"
    for bad in (torch.zeros(3), torch.zeros(1, 2), torch.zeros(2, dtype=torch.float64), torch.zeros(2, 2)[:, 0]):
        g.log_std = torch.nn.Parameter(bad)
        assert actor_path(g, N) == "host", bad                                   # shape, dtype, not contiguous
    g.log_std = torch.nn.Parameter(torch.zeros(2))
    assert actor_path(g, N, device="cuda:0") == "host"                          # not on the env's device
    assert actor_path(g, N, world_options=True) == "host"                       # per-agent props and other World options
    assert actor_path(g, N, callback=True) == "host"


def test_plain_actor_unchanged():
    from formation_gym.actor_rollout import actor_spec
    m = _mlp(9, 64)
    assert actor_spec(GaussianActor(m), 9) is None                               # actor_spec only takes the mean
    assert actor_spec(m, 9) is not None and actor_path(m, 9) == "fused"


def _describe(lib, N, H, B=4096, K=20, log_std=4096, sample=True):
    if sample:
        return describe(lib, "fg_describe_actor_sample_launch", (_fake_actor(H), log_std), N, B, K)
    return describe(lib, "fg_describe_actor_launch", (_fake_actor(H),), N, B, K)


def test_describe_names_one_sample_instantiation_per_shape():
    lib = _native.load()
    names = set()
    for N in FUSED_N:
        for H in FUSED_HIDDEN:
            rc, text = _describe(lib, N, H)
            assert rc == 0, text
            assert text.count("actor_sample_kernel<") == 1 and "actor_sample_kernel<%d,%d>" % (N, H) in text
            assert "actor_rollout_kernel" not in text
            names.add(text.split(" ")[0])
            # the same geometry as the deterministic twin; only the LDS grows (one log-prob per row)
            _, twin = _describe(lib, N, H, sample=False)
            assert text.split(" lds ")[0].split(" ", 1)[1] == twin.split(" lds ")[0].split(" ", 1)[1]
    assert len(names) == len(FUSED_N) * len(FUSED_HIDDEN)


def test_sample_status_codes_match_the_deterministic_twin():
    lib = _native.load()
    for N, H, B, K in [(81, 64, 128, 20), (9, 48, 128, 20), (9, 64, 128, 0), (9, 64, 0, 20), (9, 64, -1, 20)]:
        assert _describe(lib, N, H, B, K)[0] == _describe(lib, N, H, B, K, sample=False)[0] != 0
    assert _describe(lib, 9, 64, log_std=None)[0] == -1                      # FG_ERR_BAD_ARG: NULL log_std
    assert b"log_std" in lib.fg_last_error()
    assert _describe(lib, 9, 64, log_std=4098)[0] == -3                      # FG_ERR_ALIGNMENT


def test_sample_bad_arguments_rejected_without_a_device():
    lib = _native.load()
    f = ctypes.c_void_p(4096)

    def call(N=9, K=20, actor=None, log_std=4096, logp=4096):
        return lib.fg_rollout_hd_actor_sample(_params(), actor if actor is not None else _fake_actor(64), log_std, 128, N, K,
                                              *([f] * 12), logp, 1, None)
    assert call(log_std=None) == -1
    assert call(actor=_fake_actor(48)) == -1
    assert call(N=81) == -2
    assert call(K=0) == -1
    assert call(logp=4098) == -3
    eps = ctypes.c_void_p(4096)
    assert lib.fg_actor_noise(_params(), 16, 9, None, None) == -1
    assert lib.fg_actor_noise(_params(), 16, 9, ctypes.c_void_p(4100), None) == -3
    assert lib.fg_actor_noise(_params(), -1, 9, eps, None) == -1
    assert lib.fg_actor_noise(_params(), 0, 9, eps, None) == 0                # empty batch: a no-op, no launch


def test_sample_kernels_use_no_scratch():
    from tests.isa_scan import kernel_resources
    ks = kernel_resources(LIB)
    sample = [k for k in ks if "actor_sample_kernel<" in k["demangled"]]
    assert len(sample) == len(FUSED_N) * len(FUSED_HIDDEN)
    assert len({k["demangled"] for k in sample}) == len(sample)
    for k in sample:
        assert k["private_segment"] == 0 and k["vgpr_spill"] == 0, k
        assert k["vgpr"] <= 320, k                                                # the deterministic kernels' bound
    assert not [k for k in ks if "actor_rollout_kernel" in k["demangled"] and "actor_rollout_kernel<" not in k["demangled"]]
    noise = [k for k in ks if "actor_noise_kernel" in k["demangled"]]
    assert len(noise) == 1 and noise[0]["private_segment"] == 0


def test_distribution_methods_match_torch_normal():
    torch.manual_seed(0)
    N = 9
    mean = _mlp(N, 32).double()
    g = GaussianActor(mean, torch.nn.Parameter(torch.tensor([-0.3, 0.7], dtype=torch.float64)))
    obs = torch.randn(5, N, 6 * N, dtype=torch.float64)
    act = torch.randn(5, N, 2, dtype=torch.float64) * 2
    ref = torch.distributions.Normal(mean(obs), torch.exp(g.log_std))
    assert torch.allclose(g.log_prob(obs, act), ref.log_prob(act).sum(-1), rtol=0, atol=1e-12)
    assert torch.allclose(g.entropy(), ref.entropy()[0, 0].sum(), rtol=0, atol=1e-12)
    d = g.distribution(obs)
    assert torch.allclose(d.loc, ref.loc) and torch.allclose(d.scale, ref.scale)
    assert torch.allclose(d.log_prob(act).sum(-1), ref.log_prob(act).sum(-1), rtol=0, atol=1e-12)
    # the PPO update differentiates through log_std and the mean
    g.log_prob(obs, act).sum().backward()
    assert g.log_std.grad is not None and mean[0].weight.grad is not None
    # forward draws mean + std * eps with fresh torch noise
    a = g(obs)
    assert a.shape == (5, N, 2)
    assert GaussianActor(_mlp(N, 32)).log_std.shape == (2,) and not GaussianActor(_mlp(N, 32)).log_std.any()
