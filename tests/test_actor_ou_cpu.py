"""CPU-side tests of the OU-noise actor rollout: the path rule of `OUNoiseActor`, the C ABI of `fg_rollout_hd_actor_ou`,
`fg_rollout_hd_actor_ou_per_agent`, their describe twins and `fg_actor_ou_step` without a device, and the error model of
tests/actor_ou_testlib.py: torch's fp32 recursion stays inside the state bound 4 * 2^-24 * M / theta against fp64 over 400
steps (largest err / bound 0.15; exactly 0 at theta = 1, sigma = 0.5, where every operation is exact)."""
import ctypes
import os
import types

import pytest
import torch

import formation_gym
from formation_gym import GaussianActor, InputBatchNorm, OUNoiseActor, PerAgentActor, RecurrentActor, _native, load_scenario
from formation_gym.actor_rollout import FUSED_BN_HIDDEN, FUSED_HIDDEN, FUSED_N, FusedActor, actor_path, resolve_actor
from tests import actor_ou_testlib as ot
from tests.actor_testlib import LIB, ROOT, describe, fake_actor, fake_actors, params as _params

nn = torch.nn


def _mlp(N, H=64, tanh=False, D=None):
    D = 6 * N if D is None else D
    mods = [nn.Linear(D, H), nn.ReLU(), nn.Linear(H, H), nn.ReLU(), nn.Linear(H, 2)] + ([nn.Tanh()] if tanh else [])
    return nn.Sequential(*mods)


def _bn_mlp(N, H=64, norm=InputBatchNorm):
    return nn.Sequential(norm(6 * N), *_mlp(N, H)).eval()


def _ln_mlp(N, H=64):
    return nn.Sequential(nn.Linear(6 * N, H), nn.ReLU(), nn.LayerNorm(H), nn.Linear(H, H), nn.ReLU(), nn.LayerNorm(H),
                         nn.Linear(H, 2))


# ---- the module and the path rule ----
def test_module_defaults_initial_state_and_forward():
    assert "OUNoiseActor" in formation_gym.__all__
    ou = OUNoiseActor(_mlp(3))
    assert (ou.theta, ou.sigma, ou.scale, ou.mu, ou.clip) == (0.15, 0.2, 0.1, 0.0, 1.0)
    ou = OUNoiseActor(_mlp(3), mu=0.25, clip=None, scale=2.0, sigma=1.0)
    x = ou.initial_state(5, 3)
    assert x.shape == (5, 3, 2) and x.dtype == torch.float32 and bool((x == 0.25).all())
    torch.manual_seed(0)
    obs = torch.randn(5, 3, 18)
    act, x1 = ou(obs, x)
    assert act.shape == (5, 3, 2) and x1.shape == x.shape and bool((x == 0.25).all())        # the caller's state is not touched
    assert torch.equal(act, ou.actor(obs) + 2.0 * x1) and float(act.detach().abs().max()) > 1.0       # clip=None: no clamp
    assert ou(obs).shape == (5, 3, 2)
    clipped = OUNoiseActor(_mlp(3), scale=50.0, sigma=1.0, clip=0.5)
    a = clipped(obs)
    assert float(a.detach().abs().max()) == 0.5
    done = torch.tensor([True, False, False, True, False])
    assert ou.reset(x1, done) is x1 and bool((x1[done] == 0.25).all()) and bool((x1[~done] != 0.25).any())
    # theta = 1, mu = 0: no memory - the new state is sigma * eps whatever the old one was (maddpg-v1's noise)
    iid = OUNoiseActor(_mlp(3), theta=1.0, sigma=0.5, mu=0.0)
    torch.manual_seed(1)
    a = iid.noise_step(torch.full((4, 2), 7.0), torch.ones(4, 2))
    assert bool((a == 0.5).all())


def test_constructor_rejects_wrapped_kinds():
    rec = RecurrentActor(nn.Sequential(nn.Linear(18, 32)), nn.GRUCell(32, 32), nn.LayerNorm(32), nn.Linear(32, 2))
    for inner in (GaussianActor(_mlp(3)), rec, OUNoiseActor(_mlp(3))):
        with pytest.raises(ValueError):
            OUNoiseActor(inner)


def test_the_four_families_fuse_and_the_rest_runs_host_paced():
    N = 9
    members = PerAgentActor([_mlp(N) for _ in range(N)])
    bn_members = PerAgentActor([_bn_mlp(N, norm=nn.BatchNorm1d) for _ in range(N)]).eval()
    for inner, per_agent, has_bn in ((_mlp(N, tanh=True), False, False), (members, True, False), (_bn_mlp(N), False, True),
                                     (bn_members, True, True)):
        ou = OUNoiseActor(inner, scale=0.3)
        assert actor_path(ou, N) == "fused"
        f = resolve_actor(ou, N)
        assert isinstance(f, FusedActor) and f.ou is ou and f.log_std is None and f.per_agent is per_agent
        assert (f.in_bn is not None) is has_bn and f.norms is None and f.gru is None
        assert resolve_actor(inner, N).ou is None                                            # the defaulted field
    for H in FUSED_HIDDEN:                                                                   # the plain families' widths
        assert actor_path(OUNoiseActor(_mlp(N, H)), N) == "fused"
    assert actor_path(OUNoiseActor(_bn_mlp(N, 128)), N) == "host"
    assert actor_path(_ln_mlp(N), N) == "fused" and actor_path(OUNoiseActor(_ln_mlp(N)), N) == "host"
    assert actor_path(OUNoiseActor(_mlp(N)), N, fused_ou=False) == "host"
    assert actor_path(OUNoiseActor(_mlp(N)), N, world_options=True) == "host"
    assert actor_path(OUNoiseActor(_mlp(N).double()), N) == "host"
    t = _mlp(N)
    t[0].weight = nn.Parameter(torch.randn(6 * N, 64).t())                                   # [64, 6N], not contiguous
    assert not t[0].weight.is_contiguous() and actor_path(OUNoiseActor(t), N) == "host"
    assert actor_path(OUNoiseActor(lambda o: o[..., :2]), N) == "host"
    assert actor_path(OUNoiseActor(_bn_mlp(N).train()), N) == "host"


@pytest.mark.parametrize("name,N,L,M,num_obs,D", [("basic_formation_env", 3, 3, 0, 0, 18),
                                                  ("formation_hd_partial_env", 5, 5, 0, 3, 26),
                                                  ("formation_hd_obs_env", 4, 4, 3, 0, 28)])
def test_landmark_rule_states_no_ou_kernel(name, N, L, M, num_obs, D):
    sc = load_scenario(name)
    world = types.SimpleNamespace(agents=[None] * N, landmarks=[None] * (L + M))
    sc.num_agents, sc.num_landmarks, sc.num_obstacles, sc.num_obs, sc.obs_range = N, L, M, num_obs, 0.0
    facts = sc.actor_fused_rule(world)
    assert facts["fused_ou"] is False and facts["fused_ln_hidden"] == () and facts["in_features"] == D
    plain = _mlp(N, D=D)
    assert actor_path(plain, N, fused_scenario=True, **facts) == "fused"           # the plain body fuses there, its OU twin not
    assert actor_path(OUNoiseActor(plain), N, fused_scenario=True, **facts) == "host"


# ---- the C ABI without a device ----
ENTRIES = ("fg_rollout_hd_actor_ou", "fg_rollout_hd_actor_ou_per_agent", "fg_describe_actor_ou_launch",
           "fg_describe_actor_ou_per_agent_launch", "fg_actor_ou_step")


def _fake_ou(**kw):
    d = dict(theta=0.15, mu=0.0, sigma=0.2, scale=0.1, clip=1.0)
    d.update(kw)
    return _native.FgActorOu(**d)


def _fake_bn():
    return _native.FgActorInBn(mean=4096, var=4096, gamma=4096, beta=4096, eps=1e-5)


def test_symbols_exported_declared_and_bound():
    lib = ctypes.CDLL(LIB)
    header = open(os.path.join(ROOT, "include", "formation_hip.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _native.SIGNATURES and ("int %s(" % name) in header, name
    assert "typedef struct FgActorOu" in header
    assert _native.load().fg_abi_version() == 8                                    # an additive change


def test_struct_layout_matches_the_header(tmp_path):
    import subprocess
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "formation_hip.h"', 'int main(void){',
             'printf("size %zu\\n", sizeof(FgActorOu));']
    for fname, _ in _native.FgActorOu._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(FgActorOu, %s));' % (fname, fname))
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(_native.FgActorOu)
    for fname, _ in _native.FgActorOu._fields_:
        assert int(got[fname]) == getattr(_native.FgActorOu, fname).offset, fname


def test_actor_ou_updates_the_kept_struct():
    ou = OUNoiseActor(_mlp(3), theta=0.5, sigma=0.25, scale=0.75, mu=-1.0, clip=None)
    s = _native.actor_ou(ou)
    assert (s.theta, s.mu, s.sigma, s.scale, s.clip) == (0.5, -1.0, 0.25, 0.75, float("inf"))
    ou.scale, ou.clip = 0.125, 2.0
    assert _native.actor_ou(ou, s) is s and (s.scale, s.clip) == (0.125, 2.0)


def _call(lib, per_agent, dry, N=9, K=20, B=128, H=64, bn=False, ou="fake", state=4096):
    """(status, fg_last_error()) of the shared or per-agent OU entry (its describe twin when `dry`, which takes no state) on
    stand-in pointers; `ou`: None, or _fake_ou's keyword arguments."""
    M = max(N, 32)
    fou = None if ou is None else _fake_ou(**({} if ou == "fake" else ou))
    if per_agent:
        actor, bns = fake_actors(M, H), ((_native.FgActorInBn * M)(*[_fake_bn() for _ in range(M)]) if bn else None)
    else:
        actor, bns = fake_actor(H), (_fake_bn() if bn else None)
    if dry:
        buf = ctypes.create_string_buffer(512)
        name = "fg_describe_actor_ou_per_agent_launch" if per_agent else "fg_describe_actor_ou_launch"
        rc = getattr(lib, name)(_params(), actor, bns, fou, B, N, K, 1, buf, 512)
    else:
        name = "fg_rollout_hd_actor_ou_per_agent" if per_agent else "fg_rollout_hd_actor_ou"
        rc = getattr(lib, name)(_params(), actor, bns, fou, state, B, N, K, *([ctypes.c_void_p(4096)] * 12), 1, None)
    return rc, lib.fg_last_error().decode()


INF, NAN = float("inf"), float("nan")
# (what is wrong, status, the message after "<entry>: ")
BAD_OU = [
    (dict(ou=None), -1, "ou is NULL"),
    (dict(ou=dict(theta=-0.01)), -1, "theta must be in [0, 1]"),
    (dict(ou=dict(theta=1.01)), -1, "theta must be in [0, 1]"),
    (dict(ou=dict(theta=NAN)), -1, "theta must be in [0, 1]"),
    (dict(ou=dict(theta=INF)), -1, "theta must be in [0, 1]"),
    (dict(ou=dict(mu=NAN)), -1, "mu must be finite"),
    (dict(ou=dict(mu=-INF)), -1, "mu must be finite"),
    (dict(ou=dict(sigma=-0.1)), -1, "sigma must be finite and not negative"),
    (dict(ou=dict(sigma=INF)), -1, "sigma must be finite and not negative"),
    (dict(ou=dict(sigma=NAN)), -1, "sigma must be finite and not negative"),
    (dict(ou=dict(scale=INF)), -1, "scale must be finite"),
    (dict(ou=dict(scale=NAN)), -1, "scale must be finite"),
    (dict(ou=dict(clip=0.0)), -1, "clip must be positive (+inf: no clamp)"),
    (dict(ou=dict(clip=-1.0)), -1, "clip must be positive (+inf: no clamp)"),
    (dict(ou=dict(clip=NAN)), -1, "clip must be positive (+inf: no clamp)"),
]


def test_bad_arguments_rejected_without_a_device():
    lib = _native.load()
    whos = {False: "fg_rollout_hd_actor_ou", True: "fg_rollout_hd_actor_ou_per_agent"}
    for wrong, status, text in BAD_OU:
        for per_agent in (False, True):
            for dry in (False, True):
                for bn in (False, True):
                    rc, got = _call(lib, per_agent, dry, bn=bn, **wrong)
                    assert (rc, got) == (status, "%s: %s" % (whos[per_agent], text)), (wrong, per_agent, dry, bn, rc, got)
    for per_agent in (False, True):
        who = whos[per_agent]
        assert _call(lib, per_agent, False, state=None) == (-1, who + ": noise_state is NULL")
        assert _call(lib, per_agent, False, state=4100) == (-3, who + ": noise_state must be 8-byte aligned")
        assert _call(lib, per_agent, False, state=None, B=0)[0] == 0                        # an empty batch is a no-op
        assert _call(lib, per_agent, False, B=0)[0] == 0
        assert _call(lib, per_agent, False, B=0, ou=dict(theta=2.0))[0] == -1               # ... after the checks
        # every valid corner: theta 0 and 1, sigma 0, clip +inf, a negative scale
        for ok in (dict(theta=0.0), dict(theta=1.0), dict(sigma=0.0), dict(clip=INF), dict(scale=-0.5)):
            assert _call(lib, per_agent, False, B=0, ou=ok)[0] == 0, ok
            assert _call(lib, per_agent, True, ou=ok)[0] == 0, ok
        # what the inner entries check, with their texts, comes first
        assert _call(lib, per_agent, False, H=48, ou=None) == (-1, "fg_rollout_hd_actor: hidden must be 32, 64 or 128")
        assert _call(lib, per_agent, False, N=81, ou=None)[0] == -2 and _call(lib, per_agent, False, K=0, ou=None)[0] == -1
        member = "member 0: " if per_agent else ""
        assert _call(lib, per_agent, False, H=128, bn=True) == (-1, who + ": " + member + "hidden must be 32 or 64 with an input BatchNorm")
        assert _call(lib, per_agent, True, B=0) == (-1, "fg_describe_actor_launch: B > 0 required")
    # the helper of the host-paced loop
    step = lib.fg_actor_ou_step
    assert step(_fake_ou(), 0, None, None, None) == 0
    assert step(_fake_ou(), -1, 4096, 4096, None) == -1
    assert step(None, 4, 4096, 4096, None) == -1 and lib.fg_last_error().decode() == "fg_actor_ou_step: ou is NULL"
    assert step(_fake_ou(theta=1.5), 4, 4096, 4096, None) == -1
    assert lib.fg_last_error().decode() == "fg_actor_ou_step: theta must be in [0, 1]"
    assert step(_fake_ou(), 4, 4096, None, None) == -1 and step(_fake_ou(), 4, None, 4096, None) == -1
    assert step(_fake_ou(), 4, 4096, 4100, None) == -3 and step(_fake_ou(), 4, 4100, 4096, None) == -3


def test_describe_names_one_instantiation_per_shape_with_the_family_geometry():
    lib = _native.load()
    names = set()
    for N in FUSED_N:
        for bn in (False, True):
            for H in (FUSED_BN_HIDDEN if bn else FUSED_HIDDEN):
                for per_agent in (False, True):
                    kernel = ("pa_" if per_agent else "") + ("bn_" if bn else "") + "ou_actor_kernel"
                    if per_agent:
                        bns = (_native.FgActorInBn * N)(*[_fake_bn() for _ in range(N)]) if bn else None
                        rc, text = describe(lib, "fg_describe_actor_ou_per_agent_launch", (fake_actors(N, H), bns, _fake_ou()), N)
                        rc2, twin = (describe(lib, "fg_describe_actor_bn_per_agent_launch", (fake_actors(N, H), bns, None), N) if bn
                                     else describe(lib, "fg_describe_actor_per_agent_launch", (fake_actors(N, H), None), N))
                    else:
                        fbn = _fake_bn() if bn else None
                        rc, text = describe(lib, "fg_describe_actor_ou_launch", (fake_actor(H), fbn, _fake_ou()), N)
                        rc2, twin = (describe(lib, "fg_describe_actor_bn_launch", (fake_actor(H), fbn, None), N) if bn
                                     else describe(lib, "fg_describe_actor_launch", (fake_actor(H),), N))
                    assert rc == 0 and rc2 == 0, (text, twin)
                    assert text.startswith("%s<%d,%d> " % (kernel, N, H)) and text.count("_kernel<") == 1, text
                    geometry = lambda t: t.split("> ")[1].split(" lds ")[0]
                    assert geometry(text) == geometry(twin), (text, twin)          # grid, block, envs per workgroup
                    lds, twin_lds = (int(t.split(" lds ")[1].split(";")[0]) for t in (text, twin))
                    envs = int(text.split("envs/wg ")[1].split(" ")[0])
                    assert lds == twin_lds + 8 * envs * N and lds <= 160 * 1024, (text, twin)   # the state: [E N][2] floats
                    names.add(text.split(" ")[0])
    assert len(names) == 2 * len(FUSED_N) * (len(FUSED_HIDDEN) + len(FUSED_BN_HIDDEN)) == 80
    rc, text = describe(lib, "fg_describe_actor_ou_launch", (fake_actor(64), None, _fake_ou()), 9)
    assert text.startswith("ou_actor_kernel<9,64> ")


def test_ou_kernels_use_no_scratch():
    from tests.isa_scan import kernel_resources
    ks = kernel_resources(LIB)
    nh, nb = len(FUSED_N) * len(FUSED_HIDDEN), len(FUSED_N) * len(FUSED_BN_HIDDEN)
    for kern, count in ((" fg::ou_actor_kernel<", nh), (" fg::pa_ou_actor_kernel<", nh), (" fg::bn_ou_actor_kernel<", nb),
                        (" fg::pa_bn_ou_actor_kernel<", nb)):
        mine = [k for k in ks if kern in " " + k["demangled"]]
        assert len(mine) == count and len({k["demangled"] for k in mine}) == count, (kern, len(mine))
        for k in mine:
            assert k["private_segment"] == 0 and k["vgpr_spill"] == 0, k


# ---- the error model ----
@pytest.mark.parametrize("theta,sigma,mu", [(0.15, 0.2, 0.0), (1.0, 0.5, 0.0), (0.05, 1.0, 0.3)])
def test_fp32_recursion_stays_inside_the_state_bound(theta, sigma, mu):
    """torch's fp32 x + theta (mu - x) + sigma eps - more roundings than the kernels' two fmas - against the fp64 reference
    over 400 steps, with resets at scattered steps: err / bound at every step."""
    g = torch.Generator().manual_seed(7)
    steps, rows = 400, 512
    eps = torch.randn(steps, rows, 2, generator=g)
    done = torch.rand(steps, rows, generator=g) < 0.02
    x0 = 0.5 * torch.randn(rows, 2, generator=g)
    used64, end64 = ot.ou_reference(theta, mu, sigma, x0, eps, done)
    bound = ot.state_bound(theta, mu, sigma, used64, eps)
    x, worst = x0.clone(), 0.0
    for k in range(steps):
        x = x + theta * (mu - x) + sigma * eps[k]
        assert x.dtype == torch.float32
        worst = max(worst, float((x.double() - used64[k]).abs().max()) / bound)
        x = torch.where(done[k].unsqueeze(-1), torch.full_like(x, mu), x)
    worst = max(worst, float((x.double() - end64).abs().max()) / bound)
    print("OU fp32 recursion theta=%g sigma=%g mu=%g max err/bound = %.4f" % (theta, sigma, mu, worst))
    assert worst <= 1.0
    if theta == 1.0:
        assert worst == 0.0                                                # x - x, then a product by a power of two: exact
    # the reference can see a wrong recursion: each mutant leaves the bound by a wide margin
    for name, f in (("no mean reversion", lambda x, e: x + sigma * e), ("no memory", lambda x, e: theta * mu + sigma * e),
                    ("sigma dropped", lambda x, e: x + theta * (mu - x) + e)):
        if (theta == 1.0 and name == "no memory") or (sigma == 1.0 and name == "sigma dropped"):
            continue                                                       # not a mutant of this case
        y = x0.clone().double()
        far = 0.0
        for k in range(40):
            y = f(y, eps[k].double())
            far = max(far, float((y - used64[k]).abs().max()) / bound)
            y = torch.where(done[k].unsqueeze(-1), torch.full_like(y, mu), y)
        assert far > 10.0, (name, far)
