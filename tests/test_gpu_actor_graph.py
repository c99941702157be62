"""GPU tests of `rollout_actor` the way a trainer drives it: under the device RNG counter (`env.use_device_rng_counter()`: the
base offset is FgParams.rng_offset + *FgParams.rng_offset_dev) and replayed from a hipGraph captured once
(`fg_rollout_hd_actor*`, `fg_rollout_scenario_actor`, and the host-paced helpers `fg_actor_noise`, `fg_actor_uniform`,
`fg_actor_gumbel`).  Inputs, cases and actors: tests/actor_graph_testlib.py; tests/test_actor_graph_cpu.py shows that the
references at these offsets tell a lost carry, an offset that does not advance and a replay that repeats block 0 apart.

Blocks 0 .. 3 are one eager call and three replays of K = 3 steps from offset 2^32 - 8: the carry into the offset's high word
falls inside replay 2 and can only arrive through the counter.  world_length = 2 with auto_reset ends episodes in every block.
Between blocks 1 and 2 every parameter of the actor is multiplied by 0.9 in place (a BatchNorm's running_mean too).

(a) `test_replayed_graph_equals_by_value_launches`: everything a block returns and leaves behind - observations, rewards, done
    flags, every info tensor, the states, the simulator's state - equals, bit for bit, the same blocks launched one by one with
    by-value offsets; the counter ends at START - 1 + 4 K; after `use_device_rng_counter(False)` a fifth by-value block agrees too.
    Both sides run the same code, so an error they share stays equal: every call therefore also checks that info returns the
    caller's own state tensors (`actor_graph_testlib.block`), and the by-value side that each block leaves another state behind.
(b) `test_replayed_draws_are_the_philox_reference`: the independent anchor.  The draw-revealing actors make the launch's outputs
    the draws themselves, which every block and step holds to the NumPy Philox reference at block_offsets(r)[k]:
    Gaussian / OU  |a - eps64| <= counter_rng.gauss_bound(r) per component (the bound of tests/test_gpu_actor_sample.py: the
                   revealing actor adds exact zeros and multiplies by exact ones); the OU state a block leaves behind is the last
                   step's action, or mu = 0 where that step ended the episode.
    categorical    the index is actor_cat_testlib.pick(0, u64) outside exempt(margin, beta=0) (ETA0 = 2^-16), which may hold at
                   most 1 % of a case's rows; log_prob within 1e-6 of log 0.2; the action decodes the launch's own index.
    Gumbel         the index is actor_gumbel_testlib.pick(0, g64) outside exempt(margin, beta=0, g), at most 1 % likewise; the
                   action decodes the launch's own index.
    Each case prints its measured maxima as shares of the bounds and its exempt shares (`pytest -s`); profiles/actor_graph.md
    records them.
(c) `test_counter_split_without_a_graph`, `test_host_paced_twin_under_the_counter`: the same blocks launched eagerly with 1 by
    value and the rest in the counter (START - 1 before block 0, 2^32 - 3 before the block that carries) equal the by-value
    blocks bit for bit, fused and host-paced.
(d) `test_what_a_graph_freezes`: `ou.scale`, `cat.deterministic` and `gumbel.explore` are read on the host at every CALL, so a
    replay keeps the values of the capture while an eager call sees the new ones.
Run with `pytest -m gpu`.
"""
import functools
import math

import numpy as np
import pytest
import torch

from tests import actor_cat_testlib as ct
from tests import actor_graph_testlib as ag
from tests import counter_rng as R

pytestmark = pytest.mark.gpu

K, BLOCKS, START = ag.K, ag.BLOCKS, ag.START
ALL = pytest.mark.parametrize("case", ag.CASES, ids=ag.case_id)


def _np(t):
    return t.detach().cpu().numpy()


def _setup(c, build=ag.actor, offset=START):
    """(env, actor, out, states) of one side of a comparison; both sides build the same bits."""
    e = ag.env(c, offset)
    a = build(c)
    assert e.actor_path(a) == "fused", ag.case_id(c)
    if c.obs_dtype is not None:
        assert e.obs_path(c.obs_dtype, actor=a) == "fused"
    return e, a, ag.out_buffers(e, c, a), ag.states(c, a, revealed=build is ag.revealing)


def _between(r, a):
    """What the optimiser does before block r."""
    if r == 2:
        ag.decay(a)


def _by_value(c, build=ag.actor, blocks=BLOCKS + 1, tweak=None):
    """Blocks 0 .. blocks - 1 launched one by one with by-value offsets: the records, nothing of which is modified afterwards.
    `tweak(r, actor)` runs before block r, after the weight update."""
    e, a, out, st = _setup(c, build)
    assert e.world.rng_counter is None
    recs = []
    for r in range(blocks):
        _between(r, a)
        if tweak is not None:
            tweak(r, a)
        assert e._launch_rng_offset() == START + K * r
        recs.append(ag.record(e, ag.block(e, c, a, out, st), st))
    torch.cuda.synchronize()
    return recs


@functools.lru_cache(maxsize=None)
def _reference(c):
    """Case `c`'s by-value blocks 0 .. 4 with the real actor, computed once and shared by (a) and (c)."""
    recs = _by_value(c)
    for r in range(BLOCKS):
        assert bool(recs[r]["done"].any()) and not bool(recs[r]["done"].all()), "block %d ends no episode" % r
    assert ag.differences(recs[1], recs[0]) and ag.differences(recs[2], recs[1])
    for k in [k for k in recs[0] if k.startswith("state.")]:                 # the caller's state tensors are carried: each block
        for r in range(1, BLOCKS):                                           # leaves another state behind, the one info returns
            assert not torch.equal(recs[r][k], recs[r - 1][k]), "%s does not move from block %d to %d" % (k, r - 1, r)
            assert torch.equal(recs[r][k], recs[r]["info." + k[len("state."):]])
    return recs


def _same(got, want, what):
    diff = ag.differences(got, want)
    assert not diff, "%s: %s differ" % (what, ", ".join(diff))


def _captured(c, e, a, out, st, on_block, after_capture=None, replays=K):
    """Env `e` under the device counter: block 0 eagerly on a side stream (also the warm-up: the LDS opt-in and every lazy
    initialisation happen before the capture), ONE `rollout_actor` call captured on that stream - a linear chain - and
    replayed; `on_block(r, record)` sees what block r returned and left behind.  Returns the graph (the caller keeps it alive
    while it looks at the counter)."""
    e.use_device_rng_counter()
    assert e._launch_rng_offset() == 1 and int(e.world.rng_counter.item()) == START - 1
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        res = ag.block(e, c, a, out, st)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    on_block(0, ag.record(e, res, st))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        res = ag.block(e, c, a, out, st)                   # the tensors of `res` are out's and st's: every replay refills them
    if after_capture is not None:
        after_capture(a)
    for r in range(1, replays + 1):
        _between(r, a)
        graph.replay()
        torch.cuda.synchronize()
        on_block(r, ag.record(e, res, st))
    return graph


def _equals(ref, what):
    return lambda r, rec: _same(rec, ref[r], "%s block %d" % (what, r))


# ---------------------------------------------------------------------------------------------------------------------
# (a) the replayed graph equals the by-value launches
# ---------------------------------------------------------------------------------------------------------------------
@ALL
def test_replayed_graph_equals_by_value_launches(case):
    ref = _reference(case)
    e, a, out, st = _setup(case)
    graph = _captured(case, e, a, out, st, _equals(ref, "captured"))
    assert int(e.world.rng_counter.item()) == START - 1 + 4 * K
    e.use_device_rng_counter(False)
    assert e.world.rng_counter is None and e._launch_rng_offset() == START + 4 * K
    res = ag.block(e, case, a, out, st)
    torch.cuda.synchronize()
    _same(ag.record(e, res, st), ref[4], "the by-value block after the replays")
    del graph


# ---------------------------------------------------------------------------------------------------------------------
# (b) the draws of every replay are the Philox reference's
# ---------------------------------------------------------------------------------------------------------------------
def _check_gauss(c, recs):
    worst = 0.0
    for r in range(BLOCKS):
        eps = ag.draws(c.member, c.B, c.N, ag.block_offsets(r))                          # [K, B, N, 2]
        rad = np.sqrt((eps * eps).sum(-1, keepdims=True))
        bound = R.gauss_bound(rad)
        act = recs[r]["info.actions"]
        err = np.abs(_np(act).astype(np.float64) - eps)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), "block %d: max |a - eps64| / bound = %.3g" % (r, float((err / bound).max()))
        if c.member == "ou":
            last_done = recs[r]["done"][K - 1].reshape(c.B, c.N, 1)
            want = torch.where(last_done, torch.zeros_like(act[K - 1]), act[K - 1])
            assert torch.equal(recs[r]["state.noise_state"], want), "block %d: the OU state is not the last step's eps" % r
        else:
            a32 = act.double()
            lp = -0.5 * (a32[..., 0] ** 2 + a32[..., 1] ** 2) - math.log(2.0 * math.pi)
            assert float((recs[r]["info.log_prob"].double() - lp).abs().max()) <= 1e-6 * (1.0 + float(lp.abs().max()))
    print("actor_graph measured: case %s worst |a - eps64| / gauss_bound = %.3f" % (ag.case_id(c), worst))


def _check_picks(c, recs):
    shares, worst_lp = [], 0.0
    for r in range(BLOCKS):
        d = ag.draws(c.member, c.B, c.N, ag.block_offsets(r))
        want, ex = ag.reference_indices(c.member, d)
        idx = _np(recs[r]["info.actions"]).astype(np.int64)
        share = float(ex.mean())
        shares.append(share)
        assert share <= ag.EXEMPT_CAP, "block %d: exempt share %.4f" % (r, share)
        assert idx.shape == want.shape and int(idx.min()) >= 0 and int(idx.max()) <= 4
        assert np.array_equal(idx[~ex], want[~ex]), "block %d: %d of %d rows differ" % (r, int((idx != want)[~ex].sum()), int((~ex).sum()))
        assert np.array_equal(_np(recs[r]["info.u"]).astype(np.float64), ct.decode(c.mode, idx))      # every row
        if c.member == "cat":
            err = float((recs[r]["info.log_prob"].double() - math.log(0.2)).abs().max())
            worst_lp = max(worst_lp, err)
            assert err <= 1e-6, "block %d: log_prob off log 0.2 by %.3g" % (r, err)
        else:
            assert "info.log_prob" not in recs[r]
    print("actor_graph measured: case %s exempt shares per block %s%s" % (
        ag.case_id(c), " ".join("%.4f" % s for s in shares),
        "" if c.member != "cat" else ", worst |log_prob - log 0.2| / 1e-6 = %.3f" % (worst_lp / 1e-6)))


@pytest.mark.parametrize("case", ag.by_num(ag.REVEALING), ids=ag.case_id)
def test_replayed_draws_are_the_philox_reference(case):
    recs = []
    e, a, out, st = _setup(case, ag.revealing)
    graph = _captured(case, e, a, out, st, lambda r, rec: recs.append(rec))
    assert len(recs) == BLOCKS
    assert int(e.world.rng_counter.item()) == START - 1 + 4 * K
    for r in range(BLOCKS):
        assert bool(recs[r]["done"].any()) and not bool(recs[r]["done"].all())
    if case.member in ("gauss", "ou"):
        _check_gauss(case, recs)
    else:
        _check_picks(case, recs)
    del graph


# ---------------------------------------------------------------------------------------------------------------------
# (c) the split offset without a graph
# ---------------------------------------------------------------------------------------------------------------------
@ALL
def test_counter_split_without_a_graph(case):
    """The `rollout_actor` twin of test_hd_launch_offset_split_with_the_device_counter: 1 by value and the rest in the counter."""
    ref = _reference(case)
    e, a, out, st = _setup(case)
    e.use_device_rng_counter()
    for r in range(BLOCKS):
        _between(r, a)
        assert e._launch_rng_offset() == 1
        if r in (0, 2):                                    # block 0, and the block that carries
            assert int(e.world.rng_counter.item()) == {0: START - 1, 2: 2 ** 32 - 3}[r]
        res = ag.block(e, case, a, out, st)
        torch.cuda.synchronize()
        _same(ag.record(e, res, st), ref[r], "block %d with the offset split" % r)
    assert int(e.world.rng_counter.item()) == START - 1 + 4 * K


@pytest.mark.parametrize("case", ag.by_num(ag.HOST_TWINS), ids=ag.case_id)
def test_host_paced_twin_under_the_counter(case):
    """`_rollout_actor_by_steps` draws through actor_noise() / actor_uniform() / actor_gumbel() at `_launch_rng_offset()`, the
    constant 1 in this mode: two blocks from START and two from 2^32 - 2 (the carry) equal the by-value loop's, bit for bit."""
    runs = []
    for split in (False, True):
        recs = []
        for first in (START, 2 ** 32 - 2):
            e = ag.env(case, first)
            a = ag.host_twin(ag.actor(case))
            assert e.actor_path(a) == "host"
            st = ag.states(case, a)
            if split:
                e.use_device_rng_counter()
                assert e._launch_rng_offset() == 1 and int(e.world.rng_counter.item()) == first - 1
            for r in range(2):
                recs.append(ag.record(e, ag.block(e, case, a, False, st), st))
            if split:
                assert int(e.world.rng_counter.item()) == first - 1 + 2 * K
        runs.append(recs)
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(*runs)):
        _same(y, x, "host-paced block %d under the counter" % i)
    assert ag.differences(runs[0][1], runs[0][0]) and ag.differences(runs[0][2], runs[0][0])


# ---------------------------------------------------------------------------------------------------------------------
# (d) what a graph freezes
# ---------------------------------------------------------------------------------------------------------------------
def _new_value(a):
    """Change what the member reads on the host at every call."""
    if a.__class__.__name__ == "OUNoiseActor":
        a.scale = 0.125
    elif a.__class__.__name__ == "CategoricalActor":
        a.deterministic = True
    else:
        a.explore = False


@pytest.mark.parametrize("case", ag.by_num(ag.FROZEN), ids=ag.case_id)
def test_what_a_graph_freezes(case):
    old = _reference(case)                                                   # blocks 0 .. 4 with the captured values
    new = _by_value(case, blocks=BLOCKS, tweak=lambda r, a: _new_value(a) if r == BLOCKS - 1 else None)
    for r in range(BLOCKS - 1):
        _same(new[r], old[r], "by-value block %d" % r)
    assert ag.differences(new[3], old[3]), "the new value changes nothing: the test would see no freeze"
    e, a, out, st = _setup(case)
    graph = _captured(case, e, a, out, st, _equals(old, "captured"), after_capture=_new_value, replays=2)      # replays 1 and 2: the captured values'
    res = ag.block(e, case, a, out, st)                                      # an eager call: the new values'
    torch.cuda.synchronize()
    _same(ag.record(e, res, st), new[3], "the eager call after the replays")
    del graph
