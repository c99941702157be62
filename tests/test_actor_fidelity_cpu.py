"""CPU checks of tests/actor_fidelity.py: that the inputs and bounds of the edge tests (tests/test_gpu_actor_edges.py) can tell a
right actor from a subtly wrong one, before any kernel is involved.  The parameter sets are EDGE_SETS at
(N, H, input norm) = (9, 64, yes) and (27, 32, no), on synthetic observations of the env's layout (a zero communication block)
and states that hold exact 0 and +-1 entries (`edge_state`).

Figures on torch 2.10 (CPU), each printed before it is asserted, (9, 64) then (27, 32):
  torch's fp32 evaluation / bound (asserted <= 0.1): recurrent eps 0.025, 0.017; no_affine 0.020, 0.014; mixed 0.019, 0.013;
    mixed_no_linear_bias 0.025, 0.016; saturated (gain 27.5, 20.9) 0.0041, 0.0030; overflow (gain 183, 139) 0.0057, 0.0053;
    LayerNorm actor 0.014 to 0.029 over the four sets.  The default-weight sets carry no gain (tests/actor_fidelity.py).
  mutant / bound (asserted >= 10): the weakest is unbiased_variance - recurrent 368, 443, LayerNorm actor 487, 578; the weakest
    eps swap 642 (input / hidden 1, recurrent, (9, 64)), bhn_outside_reset 3079 and more, post_affine_ignored 6928 and more,
    input_stats_without_comm 8200 and more, hidden_affine_swap 19695 and more, rz_blocks_swapped 34928 and more, z_exchanged
    44608 and more.  With one eps for every norm each eps swap gives exactly 0.
  share of r / z pre-activations beyond 4 at GRU scale 6 (asserted > 0.2): 0.322, 0.325, the largest 18.0, 16.9; at scale 40
    the extremes are +120.3 / -107.8 and +110.9 / -112.9.
"""
import copy

import pytest
import torch

from formation_gym import RecurrentActor
from tests.actor_fidelity import (EDGE_EPS, EDGE_SETS, GAIN_SETS, NORM_BIAS_ARG, OVERFLOW_SCALE, REC_ONLY_SETS, SAT_SCALE, TOL,
                                  actor_params, edge_state, evaluate, gate_gain, ln_actor, ln_ref64, mutant_name, mutant_ratios,
                                  rec_actor, rec_bounds, rec_ref64)
from tests.actor_testlib import ACT_SCALE

nn = torch.nn
SHAPES = [(9, 64, True), (27, 32, False)]
ROWS = 48                                              # envs of the synthetic batch: 48 N rows, every `edge_state` row kind


def _obs(N, seed=5):
    """Observations [ROWS, N, 6N] of formation_hd_env's layout: velocity, relative positions, a zero communication block (units
    N .. 2N - 2), ideal shape, ideal velocity."""
    g = torch.Generator().manual_seed(seed)
    o = torch.rand((ROWS, N, 6 * N), generator=g) * 2 - 1
    o[..., :2] *= 0.3
    o[..., 2 * N:4 * N - 2] = 0.0
    return o


def _skip_without_norm_bias(name):
    if "mixed" in name and not NORM_BIAS_ARG:
        pytest.skip("this torch's LayerNorm has no `bias` argument: a norm with gamma and without beta cannot be built")


# ---- the builders build what the GPU files' own builders built ----
def _legacy_ln_actor(N, H, in_norm, tanh=False, seed=0, zero_head=False, eps=1e-5):
    """test_gpu_actor_layernorm.py's `_ln_actor` as it was before tests/actor_fidelity.py, kept here word for word."""
    torch.manual_seed(seed)
    D = 6 * N
    mods = [nn.LayerNorm(D, eps=eps)] if in_norm else []
    mods += [nn.Linear(D, H), nn.ReLU(), nn.LayerNorm(H, eps=eps), nn.Linear(H, H), nn.ReLU(), nn.LayerNorm(H, eps=eps), nn.Linear(H, 2)]
    if tanh:
        mods.append(nn.Tanh())
    m = nn.Sequential(*mods)
    with torch.no_grad():
        for mod in m:
            if isinstance(mod, nn.Linear):
                mod.weight.mul_(ACT_SCALE)
                mod.bias.mul_(ACT_SCALE)
            elif isinstance(mod, nn.LayerNorm):
                mod.weight.add_(0.25 * torch.randn_like(mod.weight))
                mod.bias.add_(0.2 * torch.randn_like(mod.bias))
        if zero_head:
            head = [mod for mod in m if isinstance(mod, nn.Linear)][-1]
            head.weight.zero_()
            head.bias.zero_()
    return m


def _legacy_rec_actor(N, H, in_norm, tanh=False, seed=0, zero_head=False, eps=1e-5):
    """test_gpu_actor_recurrent.py's `_rec_actor` as it was before tests/actor_fidelity.py, kept here word for word."""
    torch.manual_seed(seed)
    D = 6 * N
    mods = [nn.LayerNorm(D, eps=eps)] if in_norm else []
    mods += [nn.Linear(D, H), nn.ReLU(), nn.LayerNorm(H, eps=eps), nn.Linear(H, H), nn.ReLU(), nn.LayerNorm(H, eps=eps)]
    lin = nn.Linear(H, 2)
    actor = RecurrentActor(nn.Sequential(*mods), nn.GRUCell(H, H), nn.LayerNorm(H, eps=eps),
                           nn.Sequential(lin, nn.Tanh()) if tanh else lin)
    with torch.no_grad():
        for mod in actor.modules():
            if isinstance(mod, (nn.Linear, nn.GRUCell)):
                for p in mod.parameters():
                    p.mul_(ACT_SCALE)
            elif isinstance(mod, nn.LayerNorm):
                mod.weight.add_(0.25 * torch.randn_like(mod.weight))
                mod.bias.add_(0.2 * torch.randn_like(mod.bias))
        if zero_head:
            lin.weight.zero_()
            lin.bias.zero_()
    return actor


@pytest.mark.parametrize("args", [(3, 64, True, True, 0, False, 1e-5), (27, 32, False, False, 0, True, 1e-5),
                                  (9, 64, True, True, 2, False, 3e-4)])
def test_builders_with_the_old_arguments_build_the_old_bits(args):
    for new, old in ((ln_actor, _legacy_ln_actor), (rec_actor, _legacy_rec_actor)):
        a = new(*args)
        rng_new = torch.get_rng_state()
        b = old(*args)
        rng_old = torch.get_rng_state()
        assert torch.equal(rng_new, rng_old), "the new builder draws more or fewer numbers than the old one"
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and [type(m) for m in a.modules()] == [type(m) for m in b.modules()]
        assert all(torch.equal(sa[k], sb[k]) for k in sa)
        assert [m.eps for m in a.modules() if isinstance(m, nn.LayerNorm)] == [m.eps for m in b.modules()
                                                                              if isinstance(m, nn.LayerNorm)]


def test_builder_knobs_are_independent():
    N, H = 9, 32
    a = rec_actor(N, H, True, eps=EDGE_EPS, affine=(False, True, False, True), norm_bias=(True, False, True, True),
                  linear_bias=False, gru_scale=SAT_SCALE)
    lns = [m for m in a.base if isinstance(m, nn.LayerNorm)] + [a.norm]
    assert tuple(m.eps for m in lns) == EDGE_EPS
    assert [m.weight is None for m in lns] == [True, False, True, False]
    assert [getattr(m, "bias", None) is None for m in lns] == [True, True, True, False] or not NORM_BIAS_ARG
    assert all(m.bias is None for m in a.modules() if isinstance(m, nn.Linear))
    # the GRU scale touches the GRU alone; an nn.GRU member holds the GRUCell's tensors
    b = rec_actor(N, H, True, eps=EDGE_EPS)
    c = rec_actor(N, H, True, eps=EDGE_EPS, gru_scale=SAT_SCALE, gru=True)
    d = rec_actor(N, H, True, eps=EDGE_EPS, gru_scale=SAT_SCALE)
    assert isinstance(c.rnn, nn.GRU) and isinstance(b.rnn, nn.GRUCell) and isinstance(d.rnn, nn.GRUCell)
    for name in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
        assert torch.equal(getattr(c.rnn, name + "_l0"), getattr(d.rnn, name))
        assert torch.allclose(getattr(d.rnn, name), getattr(b.rnn, name) * (SAT_SCALE / ACT_SCALE), rtol=1e-6, atol=0)
    sb, sc = b.state_dict(), c.state_dict()
    assert all(torch.equal(sb[k], sc[k]) for k in sb if not k.startswith("rnn."))
    o, h = _obs(N), edge_state((ROWS, N, H))
    with torch.no_grad():
        (a_c, h_c), (a_d, h_d) = c(o, h), d(o, h)
    assert torch.equal(a_c, a_d) and torch.equal(h_c, h_d)


def test_edge_state_holds_exact_entries():
    h = edge_state((ROWS, 9, 64))
    flat = h.reshape(-1, 64)
    assert bool((flat[0::8] == 0).all()) and bool((flat[1::8] == 1).all()) and bool((flat[2::8] == -1).all())
    mixed = flat[3::8]
    assert bool((mixed == 0).any()) and bool((mixed == 1).any()) and bool((mixed == -1).any()) and bool((mixed.abs() < 1).any())
    assert float(h.abs().max()) <= 1.0


# ---- the hand-written reference is the module-based one ----
@pytest.mark.parametrize("name", sorted(EDGE_SETS))
@pytest.mark.parametrize("N,H,in_norm", SHAPES)
def test_evaluate_is_the_module_reference(N, H, in_norm, name):
    _skip_without_norm_bias(name)
    o, h = _obs(N).double(), edge_state((ROWS, N, H)).double()
    with torch.no_grad():
        ref = rec_actor(N, H, in_norm, tanh=True, **EDGE_SETS[name]).double()
        a64, h64, r1, r2, r3 = rec_ref64(ref, o, h)
        got = evaluate(actor_params(ref), o, h)
        for want, key in ((a64, "a"), (h64, "h"), (r1, "r1"), (r2, "r2"), (r3, "r3")):
            assert float(((got[key] - want).abs() / want.abs().clamp(min=1.0)).max()) <= 1e-12, key
        assert bool(torch.isfinite(a64).all()) and bool(torch.isfinite(h64).all())
        if name not in REC_ONLY_SETS:
            kw = {k: v for k, v in EDGE_SETS[name].items() if k != "gru_scale"}
            ref = ln_actor(N, H, in_norm, **kw).double()
            a64, r1, r2, _ = ln_ref64(ref, o)
            got = evaluate(actor_params(ref), o)
            for want, key in ((a64, "a"), (r1, "r1"), (r2, "r2")):
                assert float(((got[key] - want).abs() / want.abs().clamp(min=1.0)).max()) <= 1e-12, key


# ---- a right actor sits far inside the bounds ----
@pytest.mark.parametrize("name", sorted(EDGE_SETS))
@pytest.mark.parametrize("N,H,in_norm", SHAPES)
def test_fp32_evaluation_is_a_tenth_of_the_bound(N, H, in_norm, name):
    """torch's own fp32 evaluation against the fp64 reference on the same fp32 inputs: at most 0.1 of the bound, so that the
    inputs and the bound (the gain included where the set carries it) leave a right kernel a factor of ten."""
    _skip_without_norm_bias(name)
    o, h = _obs(N), edge_state((ROWS, N, H))
    gain = name in GAIN_SETS
    with torch.no_grad():
        actor = rec_actor(N, H, in_norm, **EDGE_SETS[name])
        ref = copy.deepcopy(actor).double()
        a32, h32 = actor(o, h)
        a64, h64, r1, r2, r3 = rec_ref64(ref, o.double(), h.double())
        a_bound, h_bound = rec_bounds(ref, a64, r1, r2, r3, gain=gain)
        worst = max(float(((a32.double() - a64).abs() / a_bound).max()), float(((h32.double() - h64).abs() / h_bound).max()))
        print("CPUFIDELITY rec %s N=%d H=%d gain=%.2f fp32 err/bound = %.4f" % (name, N, H, gate_gain(ref) if gain else 1.0, worst))
        assert worst <= 0.1
        if name not in REC_ONLY_SETS:
            kw = {k: v for k, v in EDGE_SETS[name].items() if k != "gru_scale"}
            actor = ln_actor(N, H, in_norm, **kw)
            a64, r1, r2, _ = ln_ref64(copy.deepcopy(actor).double(), o.double())
            bound = TOL * a64.abs().clamp(min=1.0) * r1.clamp(min=1.0) * r2.clamp(min=1.0)
            worst = float(((actor(o).double() - a64).abs() / bound).max())
            print("CPUFIDELITY ln %s N=%d H=%d fp32 err/bound = %.4f" % (name, N, H, worst))
            assert worst <= 0.1


# ---- a wrong one sits far outside ----
@pytest.mark.parametrize("N,H,in_norm", SHAPES)
def test_every_mutant_is_ten_bounds_away(N, H, in_norm):
    o, h = _obs(N), edge_state((ROWS, N, H))
    for kind, actor, state in (("rec", rec_actor(N, H, in_norm, **EDGE_SETS["eps"]), h),
                               ("ln", ln_actor(N, H, in_norm, **EDGE_SETS["eps"]), None)):
        ratios = mutant_ratios(actor, o, state)
        swaps = [m for m in ratios if m[0] == "eps_swap"]
        assert len(swaps) == {("rec", True): 6, ("rec", False): 3, ("ln", True): 3, ("ln", False): 1}[(kind, in_norm)]
        assert len(ratios) == len(swaps) + 2 + (1 if in_norm else 0) + (4 if kind == "rec" else 0)
        for m, ratio in ratios.items():
            print("CPUMUTANT %s N=%d H=%d %s err/bound = %.1f" % (kind, N, H, mutant_name(m), ratio))
        weakest = min(ratios, key=ratios.get)
        print("CPUMUTANT %s N=%d H=%d weakest: %s %.1f" % (kind, N, H, mutant_name(weakest), ratios[weakest]))
        assert ratios[weakest] >= 10.0, "the inputs cannot see %s" % mutant_name(weakest)


@pytest.mark.parametrize("N,H,in_norm", SHAPES)
def test_one_eps_for_every_norm_hides_every_swap(N, H, in_norm):
    """The gap the distinct eps close: with the former single eps every eps-swap mutant is the reference itself."""
    o, h = _obs(N), edge_state((ROWS, N, H))
    for actor, state in ((rec_actor(N, H, in_norm, eps=3e-4), h), (ln_actor(N, H, in_norm, eps=3e-4), None)):
        ratios = mutant_ratios(actor, o, state)
        swaps = [m for m in ratios if m[0] == "eps_swap"]
        assert swaps and all(ratios[m] == 0.0 for m in swaps)
        assert all(ratios[m] > 0.0 for m in ratios if m[0] != "eps_swap")


# ---- the gates are where the cases say they are ----
@pytest.mark.parametrize("N,H,in_norm", SHAPES)
def test_gates_saturate_at_scale_6_and_overflow_expf_at_scale_40(N, H, in_norm):
    o, h = _obs(N).double(), edge_state((ROWS, N, H)).double()
    with torch.no_grad():
        out = evaluate(actor_params(rec_actor(N, H, in_norm, **EDGE_SETS["saturated"]).double()), o, h)
        rz = torch.cat((out["pre_r"], out["pre_z"]), -1).abs()
        share, largest = float((rz > 4).double().mean()), float(rz.max())
        print("CPUGATES N=%d H=%d scale %g: share of |r, z pre-activation| > 4 = %.3f, largest = %.1f" % (N, H, SAT_SCALE, share, largest))
        assert share > 0.2
        # the default weights times 1.5, for the record: the near-linear regime the older cases stay in
        base = evaluate(actor_params(rec_actor(N, H, in_norm, eps=EDGE_EPS).double()), o, h)
        assert float(torch.cat((base["pre_r"], base["pre_z"]), -1).abs().max()) < largest / 2
        ref = rec_actor(N, H, in_norm, **EDGE_SETS["overflow"]).double()
        out = evaluate(actor_params(ref), o, h)
        rz = torch.cat((out["pre_r"], out["pre_z"]), -1)
        print("CPUGATES N=%d H=%d scale %g: largest r, z pre-activation = %.1f, smallest = %.1f, entries beyond 90: %d"
              % (N, H, OVERFLOW_SCALE, float(rz.max()), float(rz.min()), int((rz.abs() > 90).sum())))
        # expf(-x) in 1 / (1 + expf(-x)) overflows to inf for x < -88.7 and underflows to 0 for x > 103 (to a denormal from 87.3)
        assert bool((rz > 90).any()) and bool((rz < -90).any())
        a64, h64, _, _, r3 = rec_ref64(ref, o, h)
        assert bool(torch.isfinite(a64).all()) and bool(torch.isfinite(h64).all()) and bool(torch.isfinite(r3).all())
        assert float(h64.abs().max()) <= 1.0


# ---- the host wiring, as far as it goes without a device ----
@pytest.mark.parametrize("name", ["eps", "mixed", "mixed_no_linear_bias"])
def test_resolution_and_ctypes_mirrors_keep_every_norm_apart(name):
    """resolve_actor -> _native.actor_norm / actor_gru: each eps and each gamma / beta pointer lands in its own field, an absent
    tensor as NULL.  (What the launch does with the fields is the GPU tests'.)"""
    import ctypes
    import numpy as np
    from formation_gym import _native
    from formation_gym.actor_rollout import resolve_actor
    _skip_without_norm_bias(name)
    N, H = 9, 64
    actor = rec_actor(N, H, True, tanh=True, **EDGE_SETS[name])
    fused = resolve_actor(actor, N)
    assert fused is not None and fused.gru is not None
    lns = [m for m in actor.base if isinstance(m, nn.LayerNorm)] + [actor.norm]
    fn, fg = _native.actor_norm(fused.norms), _native.actor_gru(fused.gru)
    f32 = lambda v: float(np.float32(v))
    assert (fn.in_eps, fn.h1_eps, fn.h2_eps, fg.norm_eps) == tuple(f32(e) for e in EDGE_EPS) and fn.in_norm == 1
    addr = lambda t: None if t is None else t.data_ptr()
    want = [addr(t) for m in lns for t in (m.weight, getattr(m, "bias", None))]
    got = [fn.in_gamma, fn.in_beta, fn.h1_gamma, fn.h1_beta, fn.h2_gamma, fn.h2_beta, fg.norm_gamma, fg.norm_beta]
    assert got == want and len({a for a in want if a is not None}) == sum(a is not None for a in want)
    if name != "eps":
        assert [a is None for a in want] == [True, True, False, True, True, True, False, False]
    g = actor.rnn
    assert [fg.w_ih, fg.w_hh, fg.b_ih, fg.b_hh] == [t.data_ptr() for t in (g.weight_ih, g.weight_hh, g.bias_ih, g.bias_hh)]
    lins = [m for m in actor.base if isinstance(m, nn.Linear)] + [actor.head[0]]
    assert [addr(t) for t in fused.members[0]] == [addr(t) for m in lins for t in (m.weight, m.bias)]
    assert ctypes.sizeof(fn) == 6 * ctypes.sizeof(ctypes.c_void_p) + 16
