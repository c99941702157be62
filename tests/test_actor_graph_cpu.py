"""CPU-side checks of the inputs of tests/test_gpu_actor_graph.py (tests/actor_graph_testlib.py), without a device: where the
carry into the offset's high word falls, that the Philox references at those offsets tell the three ways a replayed launch could
draw wrongly apart, that the draw-revealing actors reveal (mean 0 and logits 0 exactly, in fp64), that the references alone keep
the exempt shares of the index comparisons under their caps, and that every actor of the GPU file resolves to a fused launch.

The mutants and the blocks they must differ in (blocks 0 .. 3: one eager call and three replays of K = 3 steps from 2^32 - 8):
  high word dropped     `Variant(offset_mask=0xFFFFFFFF)`: the carry lost on its way through the counter - block 2's last step
                        (offset 2^32) and every step of block 3; blocks 0 and 1 and block 2's first two steps are the same draws.
  offset not advanced   `Variant(advance=False)`: steps 1 and 2 of every block redraw step 0's.
  replay repeats block 0   block r evaluated at block 0's offsets (the counter not read, or not advanced): blocks 1, 2 and 3.
"""
import numpy as np
import pytest
import torch

from formation_gym.actor_rollout import FusedActor, resolve_actor
from tests import actor_cat_testlib as ct
from tests import actor_graph_testlib as ag
from tests import actor_gumbel_testlib as gt
from tests import counter_rng as R

CASES = pytest.mark.parametrize("case", ag.CASES, ids=ag.case_id)
MEMBERS = ("gauss", "cat", "gumbel")                     # (the OU member draws the Gaussian's eps)


def test_inputs_are_those_of_the_counter_tests():
    assert (ag.SEED, ag.BASE) == (R.SEED, R.BASE) and ag.K == 3 and ag.START == 2 ** 32 - 8 and ag.BLOCKS == 4
    assert [c.num for c in ag.CASES] == list(range(1, 11))
    assert [(c.N, c.B, c.H) for c in ag.CASES] == [(3, 70, 64), (9, 20, 32), (27, 11, 32), (9, 20, 64), (27, 11, 64), (3, 70, 32),
                                                   (9, 20, 64), (4, 70, 32), (3, 260, 32), (4, 260, 32)]
    assert [c.mode for c in ag.CASES[4:8]] == [ct.INDEX, ct.ONEHOT5, gt.ONEHOT5, gt.INDEX]
    assert {ag.by_num([n])[0].member for n in ag.REVEALING} == {"gauss", "ou", "cat", "gumbel"}
    assert [c.member for c in ag.by_num(ag.HOST_TWINS)] == ["gauss", "ou", "cat", "gumbel"]
    assert [c.member for c in ag.by_num(ag.FROZEN)] == ["ou", "cat", "gumbel"]


def test_the_carry_falls_inside_replay_two_and_nowhere_else():
    offs = [ag.block_offsets(r) for r in range(ag.BLOCKS)]
    assert all(isinstance(o, int) for blk in offs for o in blk)
    flat = [o for blk in offs for o in blk]
    assert flat == list(range(ag.START, ag.START + ag.K * ag.BLOCKS))              # consecutive: block r starts at START + 3 r
    assert offs[2] == [2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32]
    high = [[o >> 32 for o in blk] for blk in offs]
    assert high == [[0, 0, 0], [0, 0, 0], [0, 0, 1], [1, 1, 1]]                   # the only block with two high words is 2
    # what the device counter holds before block r with 1 by value, and after the last replay
    assert [offs[r][0] - 1 for r in range(ag.BLOCKS)] == [ag.START - 1 + ag.K * r for r in range(ag.BLOCKS)]
    assert offs[2][0] - 1 == 2 ** 32 - 3 and ag.START - 1 + 4 * ag.K == offs[3][2]      # (1 by value: the last offset drawn)


@pytest.mark.parametrize("member", MEMBERS)
@pytest.mark.parametrize("N,B", sorted({(c.N, c.B) for c in ag.CASES}))
def test_references_tell_the_three_mutants_apart(member, N, B):
    true = [ag.draws(member, B, N, ag.offsets_of(r)) for r in range(ag.BLOCKS)]
    # the named references of the members' testlibs at each block's base are these draws
    launch = {"gauss": lambda rb: np.stack([R.actor_noise(ag.SEED, ag.BASE, B, N, o) for o in R.launch_offsets(rb, ag.K)]),
              "cat": lambda rb: ct.launch_uniforms(ag.SEED, ag.BASE, B, N, rb, ag.K),
              "gumbel": lambda rb: gt.launch_gumbels(ag.SEED, ag.BASE, B, N, rb, ag.K)}[member]
    for r in range(ag.BLOCKS):
        assert np.array_equal(launch(ag.block_offsets(r)[0]), true[r]) and np.isfinite(true[r]).all()

    def differs(mut):                                                              # per block and step: any element differs
        return [[bool((mut[r][k] != true[r][k]).any()) for k in range(ag.K)] for r in range(ag.BLOCKS)]

    no, yes = [False] * 3, [True] * 3
    high = [ag.draws(member, B, N, ag.offsets_of(r, R.Variant(offset_mask=0xFFFFFFFF))) for r in range(ag.BLOCKS)]
    assert differs(high) == [no, no, [False, False, True], yes]
    stuck = [ag.draws(member, B, N, ag.offsets_of(r, R.Variant(advance=False))) for r in range(ag.BLOCKS)]
    assert differs(stuck) == [[False, True, True]] * ag.BLOCKS
    if member == "cat":                                                            # the testlib's own name for it
        assert np.array_equal(stuck[2], ct.launch_uniforms(ag.SEED, ag.BASE, B, N, ag.block_offsets(2)[0], ag.K, "offset_not_advanced"))
    if member == "gumbel":
        assert np.array_equal(stuck[2], gt.launch_gumbels(ag.SEED, ag.BASE, B, N, ag.block_offsets(2)[0], ag.K, "offset_not_advanced"))
    repeat = [true[0] for _ in range(ag.BLOCKS)]
    assert differs(repeat) == [no, yes, yes, yes]
    # and by more than the bounds the GPU test compares with: most draws of a differing step lie beyond them
    if member == "gauss":
        r_ = np.sqrt((true[2][2] ** 2).sum(-1, keepdims=True))
        assert float((np.abs(high[2][2] - true[2][2]) > R.gauss_bound(r_)).mean()) > 0.99
    elif member == "gumbel":
        assert float((np.abs(high[2][2] - true[2][2]) > gt.gamma(true[2][2])).mean()) > 0.99
    else:
        assert float((ag.reference_indices("cat", high[2][2:])[0] != ag.reference_indices("cat", true[2][2:])[0]).mean()) > 0.5


@pytest.mark.parametrize("case", ag.by_num(ag.REVEALING), ids=ag.case_id)
def test_revealing_actors_give_exact_zeros_in_fp64(case):
    a = ag.revealing(case, device=None).double()
    D = ag.obs_width(case)
    if case.scenario == "formation_hd_env":
        obs = ct.cpu_observations(case.N, min(case.B, 16))
    else:
        obs = torch.randn((16, case.N, D), generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 3.0
    assert obs.shape[-1] == D
    with torch.no_grad():
        if case.member == "gauss":
            out, ones = a.mean(obs), torch.exp(a.log_std)
            assert out.shape == obs.shape[:-1] + (2,) and bool((ones == 1.0).all())
        elif case.member == "ou":
            out = a.actor(obs)
            assert (a.theta, a.mu, a.sigma, a.scale, a.clip) == (1.0, 0.0, 1.0, 1.0, None) and out.shape == obs.shape[:-1] + (2,)
            x = torch.zeros(obs.shape[:-1] + (2,), dtype=torch.float64)
            eps = torch.randn(x.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
            assert torch.equal(a.noise_step(x, eps), eps) and torch.equal(a.explore(out, eps), eps)
        else:
            out = a.logits(obs)
            assert out.shape == obs.shape[:-1] + (5,)
        assert bool((out == 0.0).all())
    if case.member == "cat":                               # five equal probabilities: log_prob = log 0.2 whatever the index
        idx, logp, _ = ct.pick(out.numpy(), np.full(out.shape[:-1], 0.5))
        assert bool((idx == 2).all()) and np.allclose(logp, np.log(0.2), rtol=0, atol=1e-15)
    # the real actor of the same case is not degenerate: the comparison of part (a) has weights to see
    real = ag.actor(case, device=None)
    assert sum(int(p.abs().sum() > 0) for p in real.parameters()) >= 6


@pytest.mark.parametrize("case", [c for c in ag.CASES if c.member in ("cat", "gumbel")], ids=ag.case_id)
def test_references_alone_stay_under_the_exempt_caps(case):
    """The exempt shares of part (b), from the references alone, for every block: at most 1 % of the rows, and every index
    occurs, so that the comparison with the device has something to bite on."""
    for r in range(ag.BLOCKS):
        d = ag.draws(case.member, case.B, case.N, ag.block_offsets(r))
        idx, ex = ag.reference_indices(case.member, d)
        assert idx.shape == ex.shape == (ag.K, case.B, case.N)
        share = float(ex.mean())
        assert share <= ag.EXEMPT_CAP, (r, share)
        assert set(np.unique(idx[~ex]).tolist()) == {0, 1, 2, 3, 4}
        counts = np.bincount(idx.ravel(), minlength=5) / idx.size
        assert float(np.abs(counts - 0.2).max()) < 0.08, counts                    # five equal probabilities
        for mode in (ct.ONEHOT5, ct.INDEX):
            assert ct.decode(mode, idx).shape == idx.shape + (2,)
    assert ag.EXEMPT_CAP == 0.01 and ct.ETA0 == 2.0 ** -16


@CASES
def test_every_actor_of_the_gpu_file_resolves_to_a_fused_launch(case):
    facts = ag.fused_facts(case)
    real = ag.actor(case, device=None)
    f = resolve_actor(real, case.N, **facts)
    assert isinstance(f, FusedActor) and f.hidden == case.H, ag.case_id(case)
    assert (f.log_std is not None) == (case.member == "gauss") and (f.ou is not None) == (case.member == "ou")
    assert (f.cat is not None) == (case.member == "cat") and (f.gumbel is not None) == (case.member == "gumbel")
    assert (f.gru is not None) == (case.body == "gru") and (f.norms is not None) == (case.body in ("ln", "gru"))
    assert (f.in_bn is not None) == (case.body in ("bn", "pa_bn")) and f.per_agent == (case.body in ("pa", "pa_bn"))
    if case.num in ag.REVEALING:
        g = resolve_actor(ag.revealing(case, device=None), case.N, **facts)
        assert isinstance(g, FusedActor) and g.hidden == case.H
    if case.num in ag.HOST_TWINS:
        assert resolve_actor(ag.host_twin(real), case.N, **facts) is None          # the twin runs host-paced
    # the update between blocks 1 and 2 is in place: the binding's key does not move, the values do
    key, before = f.binding_key(), [t.clone() for t in f.tensors()]
    ag.decay(real)
    assert resolve_actor(real, case.N, **facts).binding_key() == key
    same = sum(int(torch.equal(t, b)) for t, b in zip(f.tensors(), before))
    assert same == len(f._in_bns()) + sum(int(not bool(b.any())) for b in before)  # each running_var, and tensors of zeros
