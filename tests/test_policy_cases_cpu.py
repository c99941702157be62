"""CPU companion of tests/test_gpu_policy_branches.py (oracle and model only, no GPU): what that test can catch depends on WHICH
branches of `ezpolicy` its inputs take, so that is pinned here.

Why this file exists: the controller's earlier inputs - the seven recorded policy_* fixtures and the seeded resets x 0.5 of
tests/test_gpu_policy.py - are about 7 600 `ezpolicy` problems with ONE formed problem (policy_n9), no active clip and no exact
tie (`test_the_earlier_inputs_reach_one_formed_problem_and_no_clip`).  The designed cases of tests/policy_testlib.py reach, in
every hierarchy: formed and unformed problems at every level, every clip side, the fallback, own-mark ranks 0, 1 and >= 2, and
each tie rule (tests/golden/policy_branches.json holds the counts); their comparison margins are >= 1e-4 (>= 1e-3 in `rank`), so
the GPU test excuses nothing; and every mutant of the model moves rows by more than ten times the GPU bound.
Regenerate the counts after an intended change of the cases:
    FG_UPDATE_POLICY_BRANCHES=1 python -m pytest tests/test_policy_cases_cpu.py
"""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import formation_oracle as O
from tests import policy_testlib as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "policy_branches.json")
IDS = ["%dx%d" % h for h in T.HIERARCHIES]
TIE_RULES = ("tie_me_other", "tie_near", "tie_far", "tie_three")


def _exact(*xs):
    return all(bool((np.asarray(x).astype(np.float32).astype(np.float64) == x).all()) for x in xs)


def census_policy(rec):
    """`ezpolicy` (a local copy of oracle.formation_oracle.ezpolicy, its argsort stable: see policy_testlib.ezpolicy_stable) that
    appends to `rec`, per problem, the branches it took."""
    def policy(obs):
        obs = np.asarray(obs, dtype=np.float64)
        n = len(obs) // 6
        ideal = obs[4 * n - 2:6 * n - 2].reshape(-1, 2)
        ideal = ideal - ideal.mean(0)
        ivel = obs[-2:]
        cur = np.append(obs[2:2 * n], [0.0, 0.0]).reshape(-1, 2)
        cur = cur - cur.mean(0)
        me = cur[-1]
        sq_me = ((me - ideal) ** 2).sum(1)
        d_me = np.sqrt(sq_me)
        order = np.argsort(d_me, kind="stable")
        r = dict(tie_me_other=0, tie_near=0, tie_far=0, tie_three=0, fallback=0, rank=-1)
        sq_all = []
        act = None
        for at, idx in enumerate(order):
            sq = ((cur - ideal[idx]) ** 2).sum(1)
            sq_all.append(sq)
            d = np.sqrt(sq)
            closest = int(np.argmin(d))
            if closest != n - 1 and d[closest] == d[-1]:                  # me ties with an other for this mark: not mine
                r["tie_me_other"] += 1
                r["tie_three"] += int((d[:-1] == d[-1]).sum() >= 2)
            if closest == n - 1 or idx == order[-1]:
                raw = 0.5 * (ideal[idx] - me)
                act = np.clip(raw, -1, 1)
                if closest == n - 1:
                    r["rank"] = at
                    # marks as near to me as this one that are mine as well: only the order decides between them
                    same = [k for k in order[at + 1:] if d_me[k] == d_me[idx]
                            and int(np.argmin(np.sqrt(((cur - ideal[k]) ** 2).sum(1)))) == n - 1]
                    r["tie_near"] += int(len(same) >= 1)
                    r["tie_three"] += int(len(same) >= 2)
                else:
                    r["fallback"] = 1
                    same = int((d_me == d_me[idx]).sum())
                    r["tie_far"] += int(same >= 2)
                    r["tie_three"] += int(same >= 3)
                break
        diff = ideal - cur
        done = np.linalg.norm(diff) < 0.01
        r.update(formed=int(done), xp=int(raw[0] > 1), xm=int(raw[0] < -1), yp=int(raw[1] > 1), ym=int(raw[1] < -1),
                 exact=_exact(ideal, cur, sq_me, (me - ideal) ** 2, np.array(sq_all), (diff ** 2).sum(), diff ** 2, raw))
        rec.append(r)
        return act + (ivel if done else 0.3 * ivel)
    return policy


def census(obs, per):
    """Branch counts of the batch obs [B, N, 6N]: (counts, actions).  `policy` is called level by level, top first."""
    N = obs.shape[1]
    L = T.levels(N, per)
    c = {k: 0 for k in ("problems", "clip_xp", "clip_xm", "clip_yp", "clip_ym", "clip_leaf", "clip_upper", "fallback", "rank0",
                        "rank1", "rank2", "inexact") + TIE_RULES}
    c.update({"%s@%d" % (k, lev): 0 for k in ("formed", "unformed") for lev in range(1, L + 1)})
    acts = []
    for o in obs:
        rec = []
        acts.append(np.array(O.get_action_bfs(census_policy(rec), list(o), per, strict=False)))
        at = 0
        for lev in range(L, 0, -1):
            for r in rec[at:at + N // per ** (lev - 1)]:
                c["problems"] += 1
                c[("formed@%d" if r["formed"] else "unformed@%d") % lev] += 1
                for s in ("xp", "xm", "yp", "ym"):
                    c["clip_" + s] += r[s]
                if r["xp"] or r["xm"] or r["yp"] or r["ym"]:
                    c["clip_leaf" if lev == 1 else "clip_upper"] += 1
                c["fallback"] += r["fallback"]
                if r["rank"] >= 0:
                    c["rank%d" % min(r["rank"], 2)] += 1
                c["inexact"] += not r["exact"]
                for k in TIE_RULES:
                    c[k] += r[k]
            at += N // per ** (lev - 1)
        assert at == len(rec)
    return c, np.stack(acts)


@pytest.fixture(scope="module")
def branch_census():
    """{(per, L): {class: counts}} of the designed cases, and that the census copy of `ezpolicy` computes the reference's actions"""
    cache = {}

    def get(per, L):
        if (per, L) not in cache:
            case, obs, sl = T.stacked(per, L)
            out = {}
            for cls, s in sl.items():
                out[cls], acts = census(obs[s], per)
                assert (acts == T.reference(per, L)[s]).all()
            cache[(per, L)] = out
        return cache[(per, L)]
    return get


@pytest.mark.parametrize("per,L", T.HIERARCHIES, ids=IDS)
def test_designed_cases_reach_every_branch(branch_census, per, L):
    c = branch_census(per, L)
    N = per ** L
    assert set(c) == set(T.CLASSES if per in T.TIE_PER else T.CLASSES[:-1])
    every = {k: sum(c[cls][k] for cls in c) for k in c["formed"]}
    for lev in range(1, L + 1):
        # formed at this level in the classes built for it, next to unformed problems of the same level
        for cls in ("formed", "threshold", "misaligned"):
            assert c[cls]["formed@%d" % lev] >= 4 and c[cls]["unformed@%d" % lev] >= 4, (cls, lev, c[cls])
        assert c["rank"]["formed@%d" % lev] == 0 and c["clip"]["formed@%d" % lev] == 0
    for side in ("xp", "xm", "yp", "ym"):
        assert c["clip"]["clip_" + side] >= 4, c["clip"]
    assert c["clip"]["clip_leaf"] >= 4 and (L == 1 or c["clip"]["clip_upper"] >= 4)
    assert c["rank"]["rank0"] >= 4
    if per > 2:
        assert c["rank"]["fallback"] >= 4 and c["rank"]["rank1"] >= 4 and c["rank"]["rank2"] >= 2, c["rank"]
    else:                     # two sub-groups mirror each other about their mean: my nearer mark is mine unless distances tie
        assert every["fallback"] == c["ties"]["fallback"] > 0 and every["rank1"] == c["ties"]["rank1"]
    for cls in c:
        if cls != "ties":
            assert all(c[cls][k] == 0 for k in TIE_RULES), (cls, c[cls])
    if per in T.TIE_PER:
        t = c["ties"]
        assert t["inexact"] == 0, "a compared quantity of the ties class is not a fp32 number"
        assert t["tie_me_other"] >= 4 and t["tie_far"] >= 4, t
        # two marks equally near me and both mine, and any three-way tie, need a third sub-group
        assert per == 2 or (t["tie_near"] >= 4 and t["tie_three"] >= 2), t
    assert every["problems"] == sum(len(T.cases(per, L)[cls]["pos"]) for cls in c) * sum(N // per ** l for l in range(L))


def test_branch_counts_match_the_committed_table(branch_census):
    now = {"%d,%d" % h: branch_census(*h) for h in T.HIERARCHIES}
    if os.environ.get("FG_UPDATE_POLICY_BRANCHES"):
        _update(census=now)
    with open(GOLDEN) as fh:
        want = json.load(fh)["census"]
    assert now == want, "the case sets changed: regenerate tests/golden/policy_branches.json"


def _update(**kw):
    doc = {}
    if os.path.exists(GOLDEN):
        with open(GOLDEN) as fh:
            doc = json.load(fh)
    doc.update(kw)
    with open(GOLDEN, "w") as fh:
        json.dump(doc, fh, indent=0, sort_keys=True)


@pytest.mark.parametrize("per,L", T.HIERARCHIES, ids=IDS)
def test_model_equals_the_oracle_and_margins_need_no_exemption(per, L):
    """mutant=None IS the oracle, bit for bit, on every case; `O.ezpolicy` itself (whatever its argsort does at ties) gives the
    shared reference outside the ties class; and no row outside it sits within 1e-4 of another decision (1e-3 in `rank`; the
    threshold class is 1e-3 from the 0.01 by construction)."""
    case, obs, sl = T.stacked(per, L)
    want = T.reference(per, L)
    assert (T.model(obs, per) == want).all()
    assert (T.model(obs[0], per) == want[0]).all()                     # one env, the oracle's own calling convention
    for cls, s in sl.items():
        if cls == "ties":
            continue
        for b in range(s.start, s.stop):
            gaps = []                                              # one walk: `O.bfs_margins(...).min()` and the actions

            def policy(inp):
                gaps.append(O.ezpolicy_margin(inp))
                return O.ezpolicy(inp)
            assert (np.array(O.get_action_bfs(policy, list(obs[b]), per, strict=False)) == want[b]).all()
            m = min(gaps)
            assert m >= (1e-3 if cls == "rank" else 9e-4 if cls == "threshold" and per ** L <= 64 else 1e-4), (cls, b, m)
    for k in ("pos", "shape", "ivel"):
        assert (case[k].astype(np.float32).astype(np.float64) == case[k]).all()


# mutant -> the classes built for its branch; (needs more than one level, needs more than two sub-groups)
MUTANT_CLASSES = {
    "natural_alignment": (("formed", "misaligned"), False, False),
    "always_unformed": (("formed", "threshold"), False, False),
    "weights_swapped": (("formed", "rank"), False, False),
    "threshold_0.1": (("threshold",), False, False),
    "threshold_unsquared": (("threshold",), False, False),
    "no_clip": (("clip",), False, False),
    "clip_after_velocity": (("clip",), False, False),
    "me_wins_ties": (("ties",), False, False),
    "far_lowest_tie": (("ties",), False, False),
    "order_highest_first": (("ties",), False, True),
    "fallback_nearest": (("rank",), False, True),
    "level_factor_dropped": (("formed", "rank"), True, False),
    "level_factor_before_add": (("formed", "rank"), True, False),
    "sum_not_mean": (("formed", "rank"), True, False),
    "ideal_not_centred": (("formed", "rank"), False, False),
    "mean_over_others_only": (("formed", "rank"), False, False),
    "parent_of_wrong_group": (("formed", "rank"), True, False),
}


def moved_rows(per, L):
    """{mutant: {class: rows the mutant moves by more than ten times the GPU bound}} over every class of the hierarchy"""
    case, obs, sl = T.stacked(per, L)
    want = T.reference(per, L)
    tol = 10 * T.bound(want)[:, None]
    out = {}
    for m in T.MUTANTS:
        far = np.abs(T.model(obs, per, m) - want).max(-1) > tol
        out[m] = {cls: int(far[s].sum()) for cls, s in sl.items()}
    return out


@pytest.fixture(scope="module")
def mutant_table():
    cache = {}

    def get(per, L):
        if (per, L) not in cache:
            cache[(per, L)] = moved_rows(per, L)
        return cache[(per, L)]
    return get


@pytest.mark.parametrize("per,L", T.HIERARCHIES, ids=IDS)
def test_every_mutant_moves_rows_of_its_classes(mutant_table, per, L):
    """A device controller that carried the mutant's rule would leave the bound of the GPU test on at least 8 rows of EACH class
    built for that rule, in every hierarchy where the rule exists; the tie rules show in the ties class and nowhere else."""
    moved = mutant_table(per, L)
    assert set(MUTANT_CLASSES) == set(T.MUTANTS)
    for m, (classes, deep, wide) in MUTANT_CLASSES.items():
        for cls in classes:
            if cls == "ties" and per not in T.TIE_PER:
                continue
            if (deep and L == 1) or (wide and per == 2):
                assert moved[m][cls] == 0, (m, cls, moved[m])          # the rule does not exist here
                continue
            assert moved[m][cls] >= 8, (m, cls, moved[m])
        if m in T.TIE_MUTANTS:
            assert all(n == 0 for cls, n in moved[m].items() if cls != "ties"), (m, moved[m])


def test_mutant_table_matches_the_committed_one(mutant_table):
    now = {"%d,%d" % h: mutant_table(*h) for h in T.HIERARCHIES}
    if os.environ.get("FG_UPDATE_POLICY_BRANCHES"):
        _update(mutants=now)
    with open(GOLDEN) as fh:
        want = json.load(fh)["mutants"]
    assert now == want, "the case sets or the model changed: regenerate tests/golden/policy_branches.json"


# --------------------------------------------------------------------------------------------------------------
# the inputs the controller had before
# --------------------------------------------------------------------------------------------------------------

EARLIER_FIXTURES = ["policy_n3", "policy_n9", "policy_n27", "policy_n81", "policy_n8_per2", "policy_n16_per4", "policy_n5_per5"]
EARLIER_RANDOM = [(8, 2, 40), (16, 4, 33), (25, 5, 20), (64, 8, 9), (5, 5, 64), (7, 7, 10)]


def earlier_inputs(golden):
    """(name, per, fp64 observations [T, N, 6N]): every recorded step of the five small fixtures, 25 evenly spaced ones of
    policy_n27 / policy_n81, and six of the random cases of test_policy_kernel_other_hierarchies_against_oracle"""
    for name in EARLIER_FIXTURES:
        g = golden(name)
        per = int(g["per"]) if "per" in g else 3
        Tn = g["act"].shape[0]
        pos = np.stack([g["pos0"]] + [g["pos"][t] for t in range(Tn - 1)])
        vel = np.stack([g["vel0"]] + [g["vel"][t] for t in range(Tn - 1)])
        obs = O.observation_hd(pos, vel, np.broadcast_to(g["ideal_shape"], pos.shape), np.broadcast_to(g["ideal_vel"], (Tn, 2)))
        if pos.shape[1] >= 27:
            obs = obs[np.linspace(0, Tn - 1, 25).astype(int)]
        yield name, per, obs
    for N, per, B in EARLIER_RANDOM:
        st = O.reset_hd(7 + 1000 * np.arange(B), N)
        f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
        obs = O.observation_hd(f32(st["pos"] * 0.5), st["vel"], f32(st["ideal_shape"]), f32(st["ideal_vel"]))
        yield "random N=%d per=%d" % (N, per), per, f32(obs)


def test_the_earlier_inputs_reach_one_formed_problem_and_no_clip(golden):
    """The fact behind this file, not a requirement: over about 7 600 problems of the earlier inputs one is formed, none clips,
    none ties and none ranks its own mark third."""
    total = {}
    for name, per, obs in earlier_inputs(golden):
        c, _ = census(obs, per)
        c["formed"] = sum(v for k, v in c.items() if k.startswith("formed@"))
        for k, v in c.items():
            if "@" not in k:
                total[k] = total.get(k, 0) + v
        assert c["formed"] == (1 if name == "policy_n9" else 0), (name, c)
    print(total)
    assert total["problems"] > 4000 and total["formed"] == 1
    assert total["clip_leaf"] == total["clip_upper"] == 0
    assert all(total[k] == 0 for k in TIE_RULES)


# --------------------------------------------------------------------------------------------------------------
# the launches the GPU test reaches (no device needed)
# --------------------------------------------------------------------------------------------------------------

def test_the_closed_loop_shapes_reach_the_kernels_with_the_controller_inside():
    from formation_gym import _native
    _native.build()
    lib = _native.load()
    params = _native.FgParams(dt=0.1, damping=0.25, contact_force=100.0, contact_margin=1e-3, sensitivity=5.0, mass=1.0,
                              dist_min=0.03, collide_thresh=0.015, world_length=100, auto_reset=0)

    def describe(B, N, per):
        buf = ctypes.create_string_buffer(2048)
        assert lib.fg_describe_launch(params, None, B, N, 2, per, 1, 0, buf, len(buf)) == 0
        return buf.value.decode().strip()
    for per, L in T.CLOSED_LOOP:
        N = per ** L
        d = describe(T.CLOSED_LOOP_BATCH, N, per)
        name, args = d.split("<")[0], d.split("<")[1].split(">")[0].split(",")
        assert name == ("rollout_kernel_wide" if N >= 81 else "rollout_kernel") and int(args[0]) == N, d
        assert int(args[-2]) == per, d                              # PER != 0: the controller is compiled into the kernel
        assert "chained" not in d
    assert describe(T.LANE_BATCH, 3, 3).startswith("hd_lane_kernel<3,3,")
    assert describe(T.LANE_BATCH, 4, 2).startswith("hd_lane_kernel<4,2,")
    for per, L in T.CHAINED:
        d = describe(T.CLOSED_LOOP_BATCH, per ** L, per)
        assert d.startswith("policy_state_kernel<%d>" % per) and d.endswith("x 2 chained;"), d
