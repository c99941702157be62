"""Designed inputs for the built-in controller (`ezpolicy` expanded by `get_action_BFS`, csrc/fg_policy_kernels.hpp) and a
mutable fp64 model of it.

The controller's other tests feed it recorded trajectories and seeded resets x 0.5: about 7 600 `ezpolicy` problems of which
ONE is formed (w = 1), none clips and none ties.  The case builders here place the sub-group centroids so that every decision
branch is taken, in every hierarchy (per, L), N = per^L; tests/test_policy_cases_cpu.py pins on the CPU that they do (branch
census, margins, mutant sensitivity) and tests/test_gpu_policy_branches.py holds every device implementation to the fp64
oracle on them with no excused row.

Classes (`cases(per, L)[cls]` -> dict(pos [B,N,2], shape [B,N,2], ivel [B,2]), values rounded to fp32):
  formed      sub-group i of every group of the chosen levels sits so that the REFERENCE's alignment is formed: the s-th other
              sub-group (index order, i skipped) on ideal centroid s, me on ideal centroid per-1.  i = 0, middle, per-1; formed at
              the top only (formed parent over unformed children), at the leaves only (the reverse), at every level
  threshold   formed, then one other sub-group pushed so that the norm is 0.009 / 0.011
  misaligned  formed under the NATURAL alignment (sub-group k on centroid k: formed for the reference only where i = per-1) and
              formed for the reference at i < per-1 (never under the natural one)
  clip        |0.5 (mark - me)| > 1 in x only, y only, both, both signs, at every level
  rank        no centroid near its mark: my mark first, second, third or later in the order, and the fallback (no mark is mine:
              the last of the order); every comparison margin >= 1e-3
  ties        per in {2, 4, 8}: coordinates on a dyadic grid, every sub-group's offsets summing to zero, so that every quantity
              a decision compares is exact in fp32 and a tie is a tie in both precisions: me ties with an other for a mark, two
              marks equally near me, two marks equally far in the fallback, three-way ties
"""
import functools

import numpy as np

from oracle import formation_oracle as O

ATOL = 1e-5                                              # tests/test_gpu_policy.py: ATOL with scale_with_magnitude
CLASSES = ("formed", "threshold", "misaligned", "clip", "rank", "ties")
TIE_PER = (2, 4, 8)

# (per, L).  Stand-alone launches: per 3 .. 8 at one level (formation_hd_env takes N >= 3, so per = 2 starts at two levels) and
# the deeper ones; the closed loop: every (N, per) of tests/test_dispatch_snapshot.py's PER plus (4,4), (8,8), (64,2), (64,8);
# (6,2) is the chained-launch hierarchy.
STANDALONE = [(3, 1), (4, 1), (5, 1), (6, 1), (7, 1), (8, 1), (2, 2), (2, 3), (2, 5), (3, 2), (3, 3), (3, 5), (4, 2), (4, 3),
              (5, 2), (5, 3), (8, 2)]
CLOSED_LOOP = [(3, 1), (2, 2), (2, 3), (3, 2), (4, 2), (5, 2), (3, 3), (2, 5), (4, 3), (3, 4), (5, 3), (3, 5),
               (4, 1), (8, 1), (2, 6), (8, 2)]
CHAINED = [(6, 2)]
CLOSED_LOOP_BATCH = 64                                   # the smallest batch of the snapshot: the pipelined closed-loop kernels
LANE_BATCH = 32768                                       # 3 and 4 agents: one env per lane, the controller on registers
HIERARCHIES = sorted(set(STANDALONE + CLOSED_LOOP + CHAINED), key=lambda h: (h[0] ** h[1], h[0]))

MUTANTS = ("natural_alignment", "always_unformed", "weights_swapped", "threshold_0.1", "threshold_unsquared", "no_clip",
           "clip_after_velocity", "me_wins_ties", "far_lowest_tie", "order_highest_first", "fallback_nearest",
           "level_factor_dropped", "level_factor_before_add", "sum_not_mean", "ideal_not_centred", "mean_over_others_only",
           "parent_of_wrong_group")
TIE_MUTANTS = ("me_wins_ties", "far_lowest_tie", "order_highest_first")


def levels(N, per):
    L = int(round(np.log(N) / np.log(per)))
    assert per ** L == N, (N, per)
    return L


def bound(want):
    """The GPU bound per env: 1e-5 x max(1, the env's largest action component); want [..., N, 2]."""
    return ATOL * np.maximum(1.0, np.abs(want).max((-1, -2)))


# --------------------------------------------------------------------------------------------------------------
# the model: `O.get_action_bfs(O.ezpolicy, obs, per, strict=False)` over a batch, every rule of it one named switch
# --------------------------------------------------------------------------------------------------------------

def ezpolicy_stable(obs):
    """`O.ezpolicy` with the argsort of its line :35 asked to be stable - the one difference, and one only at exact ties.
    np.argsort's default 'quicksort' was an insertion sort for a handful of elements, hence stable, in every NumPy up to 1.x and
    still is on CPUs without AVX2 / AVX-512; NumPy 2 hands float64 argsorts of four or more elements to a vectorised sorting
    network there, which orders equal distances as it pleases.  The device controller (and `model`) keep the insertion sort's
    rule - equal distances in index order - so the `ties` class is held to this copy; wherever no two distances are equal it IS
    `O.ezpolicy` (tests/test_policy_cases_cpu.py compares the two on every other class)."""
    obs = np.asarray(obs, dtype=np.float64)
    n = len(obs) // 6
    ideal = obs[4 * n - 2:6 * n - 2].reshape(-1, 2)
    ideal = ideal - ideal.mean(0)
    ivel = obs[-2:]
    cur = np.append(obs[2:2 * n], [0.0, 0.0]).reshape(-1, 2)
    cur = cur - cur.mean(0)
    me = cur[-1]
    order = np.argsort(np.sqrt(((me - ideal) ** 2).sum(1)), kind="stable")
    act = None
    for idx in order:
        closest = int(np.argmin(np.sqrt(((cur - ideal[idx]) ** 2).sum(1))))
        if closest == n - 1 or idx == order[-1]:
            act = np.clip(0.5 * (ideal[idx] - me), -1, 1)
            break
    done = np.linalg.norm(ideal - cur) < 0.01
    return act + (ivel if done else 0.3 * ivel)


def _seq_sum(x, axis):
    """x summed along `axis` element by element, in index order (what np.mean over the first axis of a [n, 2] array does)."""
    x = np.moveaxis(x, axis, 0)
    s = x[0].copy()
    for c in range(1, x.shape[0]):
        s = s + x[c]
    return s


def _f32_exact(*xs):
    """per env: every value of every array is a fp32 number"""
    ok = True
    for x in xs:
        ok = ok & (x.astype(np.float32).astype(np.float64) == x).reshape(x.shape[0], -1).all(1)
    return ok


def _ez(others, tgt, ivel, i, m, info):
    """`ezpolicy` (oracle.formation_oracle.ezpolicy) on a batch: others [B, per-1, 2], tgt [B, per, 2], ivel [B, 2].
    Returns (act before the ideal-velocity term, weight of that term)."""
    B, per = tgt.shape[0], tgt.shape[1]
    ideal = tgt if m == "ideal_not_centred" else tgt - (_seq_sum(tgt, 1) / per)[:, None]
    cur = np.concatenate((others, np.zeros((B, 1, 2))), 1)
    cur = cur - (_seq_sum(cur, 1) / ((per - 1) if m == "mean_over_others_only" else per))[:, None]
    me = cur[:, -1]
    sq_me = ((me[:, None] - ideal) ** 2).sum(-1)                           # [B, mark]
    sq_all = ((cur[:, :, None] - ideal[:, None]) ** 2).sum(-1)             # [B, agent, mark]
    d_me, d_oth = np.sqrt(sq_me), np.sqrt(sq_all[:, :-1]).min(1)
    mine = (d_me <= d_oth) if m == "me_wins_ties" else (d_me < d_oth)      # np.argmin: first minimum, me is last
    order = np.argsort(d_me, 1, kind="stable")
    last = order[:, -1]
    if m == "far_lowest_tie":
        last = np.argmax(d_me, 1)
    if m == "order_highest_first":
        order = per - 1 - np.argsort(d_me[:, ::-1], 1, kind="stable")
    mine_sorted = np.take_along_axis(mine, order, 1)
    fallback = ~mine_sorted.any(1)
    rank = mine_sorted.argmax(1)
    pick = np.where(fallback, order[:, 0] if m == "fallback_nearest" else last, np.take_along_axis(order, rank[:, None], 1)[:, 0])
    raw = 0.5 * (ideal[np.arange(B), pick] - me)
    cur_cmp = cur
    if m == "natural_alignment":                                           # sub-group k against centroid k, me against centroid i
        cur_cmp = np.concatenate((cur[:, :i], cur[:, -1:], cur[:, i:-1]), 1)
    nsq = ((ideal - cur_cmp) ** 2).reshape(B, -1).sum(1)
    norm = np.sqrt(nsq)
    done = norm < (0.1 if m == "threshold_0.1" else 1e-4 if m == "threshold_unsquared" else 0.01)
    if m == "always_unformed":
        done = np.zeros(B, bool)
    w = np.where(done, 0.3, 1.0) if m == "weights_swapped" else np.where(done, 1.0, 0.3)
    if info is not None:
        gaps = [np.abs(d_me - d_oth).min(1), np.abs(norm - 0.01)]
        if per > 1:
            gaps.append(np.diff(np.sort(d_me, 1), axis=1).min(1))
        info["margin"] = np.minimum(info["margin"], np.min(gaps, 0))
        info["exact"] &= _f32_exact(ideal, cur, sq_me, sq_all, nsq[:, None], raw, (me[:, None] - ideal) ** 2,
                                    (cur[:, :, None] - ideal[:, None]) ** 2)
        info["fallback"] += fallback
        for r in range(3):
            info["rank%d" % r] += ~fallback & ((rank == r) if r < 2 else (rank >= 2))
        info["formed"] += done
        info["clipped"] += (np.abs(raw) > 1).any(1)
    return raw, w


def model(obs, per, mutant=None, info=None):
    """fp64 `get_action_BFS(ezpolicy, obs, per)`; obs [N, 6N] or [B, N, 6N] -> actions [N, 2] / [B, N, 2].  mutant=None equals
    `O.get_action_bfs(O.ezpolicy, ..., strict=False)` exactly (tests/test_policy_cases_cpu.py); a mutant changes the one rule its
    name says.  info: a dict that receives per-env facts the case builders select by (smallest comparison margin, fp32 exactness
    of everything compared, counts of fallback / rank / formed / clipped problems)."""
    assert mutant is None or mutant in MUTANTS, mutant
    obs = np.asarray(obs, dtype=np.float64)
    single = obs.ndim == 2
    if single:
        obs = obs[None]
    B, N = obs.shape[:2]
    levels(N, per)
    m = mutant
    if info is not None:
        info.update(margin=np.full(B, np.inf), exact=np.ones(B, bool))
        for k in ("fallback", "rank0", "rank1", "rank2", "formed", "clipped"):
            info[k] = np.zeros(B, int)
    act = np.empty((B, N, 2))
    queue = [(0, N, None)]
    while queue:
        g0, n_cur, tv = queue.pop(0)
        n_sub = n_cur // per
        level = np.log(n_cur) / np.log(per)                  # the reference's float: 4.999999999999999 at 243 agents
        div = 1.0 if (m == "sum_not_mean" and n_sub > 1) else float(n_sub)
        subs = []
        for i in range(per):
            a = g0 + i * n_sub                               # the sub-group's leader and its own observation row
            oth = obs[:, a, 2:2 * N].reshape(B, N - 1, 2)
            rel = np.concatenate((oth[:, g0:a], np.zeros((B, 1, 2)), oth[:, a:g0 + n_cur - 1]), 1)
            cent = _seq_sum(rel.reshape(B, per, n_sub, 2), 2) / div
            cent = np.delete(cent - cent[:, i:i + 1], i, 1)
            shp = obs[:, a, 4 * N - 2:6 * N - 2].reshape(B, N, 2)[:, g0:g0 + n_cur]
            tgt = _seq_sum(shp.reshape(B, per, n_sub, 2), 2) / div
            ivel = obs[:, a, -2:] if tv is None else tv
            raw, w = _ez(cent, tgt, ivel, i, m, info)
            if m == "no_clip":
                sub = raw + w[:, None] * ivel
            elif m == "clip_after_velocity":
                sub = np.clip(raw + w[:, None] * ivel, -1, 1)
            else:
                sub = np.clip(raw, -1, 1) + np.where(w[:, None] == 1.0, ivel, w[:, None] * ivel)
            if m == "level_factor_before_add":
                sub = np.clip(raw, -1, 1) * level + w[:, None] * ivel
            elif m != "level_factor_dropped":
                sub = sub * level
            subs.append(sub)
        for i in range(per):
            if n_sub == 1:
                act[:, g0 + i] = subs[i]
            else:
                queue.append((g0 + i * n_sub, n_sub, subs[(i + 1) % per] if m == "parent_of_wrong_group" else subs[i]))
    return act[0] if single else act


# --------------------------------------------------------------------------------------------------------------
# case builders
# --------------------------------------------------------------------------------------------------------------

def _f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def observations(case):
    """What the controller sees: fp64 observations [B, N, 6N] of the case's fp32 values (zero velocities), rounded to fp32 -
    `p_k - p_j` of two fp32 numbers rounds to the fp32 subtraction the observation writers and the state-based launch perform."""
    pos = case["pos"]
    return _f32(O.observation_hd(pos, np.zeros_like(pos), case["shape"], case["ivel"]))


def _compose(tabs, per, L):
    """tabs[l] [B, per^l groups, per, 2] (l = 0: the top level) -> points [B, N, 2]: agent a = sum over levels of its entry"""
    B = tabs[0].shape[0]
    return sum(np.repeat(tabs[l].reshape(B, per ** (l + 1), 2), per ** (L - 1 - l), axis=1) for l in range(L))


def _sigma(per, i):
    """the reference's alignment as a permutation: sub-group k sits on ideal centroid sigma[k] (me = i on per-1)"""
    return np.array([k if k < i else per - 1 if k == i else k - 1 for k in range(per)])


_UNIT = np.array([[1.0, 0.0], [0.0, 1.0], [0.6, 0.8], [0.8, 0.6]])       # push directions (no libm call: the cases are the same bits everywhere)


def _arrange(rng, shape, per, L, plan):
    """Positions [B, N, 2] from the shape: level by level, leaves first, every group's sub-groups are shifted as wholes so that
    their centroids sit where plan[b][l] = (kind, i, amp, push) says: 'formed' - on the ideal centroids permuted by the
    reference's alignment for sub-group i (inside a group a permutation leaves the centroid where it is); 'natural' - on their
    own; 'unformed' - their own plus a displacement of up to amp (x, y).  push = (norm, k): sub-group k then leaves by a vector
    that makes ||ideal - cur|| = norm for sub-group i's problem (|d| = norm sqrt(per / (per - 1)); k = i moves me)."""
    B, N = shape.shape[:2]
    pos = shape + rng.uniform(-1, 1, (B, 1, 2))
    for l in range(L - 1, -1, -1):
        G, n_sub = per ** l, per ** (L - 1 - l)
        P = pos.reshape(B, G, per, n_sub, 2).copy()
        cS = shape.reshape(B, G, per, n_sub, 2).mean(3)
        cP = P.mean(3)
        for b in range(B):
            kind, i, amp, push = plan[b][l]
            want = cS[b][:, _sigma(per, i)] if kind == "formed" else cS[b].copy()
            if kind == "unformed":
                want = want + rng.uniform(-1, 1, want.shape) * np.asarray(amp)
            if push is not None and push[0] == "toward":    # me, a fraction of the way towards the middle of the others
                k = push[1]
                want[:, k] += push[2] * ((want.sum(1) - want[:, k]) / (per - 1.0) - want[:, k])
            elif push is not None:
                unit = _UNIT[rng.randint(0, len(_UNIT), G)] * rng.choice([-1.0, 1.0], (G, 2))
                want[:, push[1]] += push[0] * np.sqrt(per / (per - 1.0)) * unit
            want = want + (cP[b].mean(1, keepdims=True) - want.mean(1, keepdims=True))
            P[b] += (want - cP[b])[:, :, None, :]
        pos = P.reshape(B, N, 2)
    return pos


def _where(where, l, L):
    return where == "all" or (where == "top" and l == 0) or (where == "leaf" and l == L - 1)


def _plans(cls, per, L):
    """the variants of a class: each a list over levels (top first) of (kind, i, amp, push)"""
    idx = sorted({0, per // 2, per - 1})
    wheres = ["all", "top", "leaf"] if L > 1 else ["all"]
    un = ("unformed", 0, (0.7, 0.7), None)
    out = []
    if cls == "formed":
        for w in wheres:
            for i in idx:
                out.append([("formed", i, None, None) if _where(w, l, L) else un for l in range(L)])
    elif cls == "misaligned":
        for w in wheres:
            out.append([("natural", 0, None, None) if _where(w, l, L) else un for l in range(L)])
        for i in idx[:-1]:
            out.append([("formed", i, None, None)] * L)
    elif cls == "threshold":
        for i in idx:
            for lp in sorted({0, L - 1}):
                for norm in (0.009, 0.011):
                    k = (i + 1 + (lp + i) % (per - 1)) % per                      # some other sub-group
                    out.append([("formed", i, None, (norm, k) if l == lp else None) for l in range(L)])
        out = out[::5] + [p for n, p in enumerate(out) if n % 5]                  # a short prefix still mixes i, level, side
    elif cls == "clip":
        for amp in ((5.0, 0.4), (0.4, 5.0), (5.0, 5.0)):
            out.append([("unformed", 0, amp, None)] * L)
    elif cls == "rank":
        out.append([("unformed", 0, (1.5, 1.5), None)] * L)
        out.append([("unformed", 0, (3.0, 3.0), None)] * L)
        # the others on the first per-1 ideal centroids and me far from the last one: the marks nearest to me belong to others
        for i in idx:
            for far in (1.0, 2.0):
                out.append([("formed", i, None, (far, i))] * L)
            for part in (0.65, 0.85):                       # ... me nearer to the others' marks than to mine, which is still mine
                out.append([("formed", i, None, ("toward", i, part))] * L)
    return out


def _n_envs(N):
    return 16 if N <= 64 else 8 if N <= 81 else 6


def _ivel(rng, B):
    return rng.choice([-1.0, 1.0], (B, 2)) * rng.uniform(0.3, 1.0, (B, 2))


def _designed(cls, per, L, seed):
    N, n = per ** L, _n_envs(per ** L)
    rng = np.random.RandomState(seed)
    plans = _plans(cls, per, L)
    floor = 1e-3 if (cls == "rank" or N <= 64) else 2e-4
    if cls == "threshold":
        floor = min(floor, 9e-4)
    kept, infos, v = [], [], 0
    pool = n * ((8 if N <= 27 else 4) if cls == "rank" else 1)                  # rank: the envs with fallbacks and late own marks, chosen from a pool
    for _ in range(400):
        B = 16 if N <= 64 else 8
        tabs = [np.round(rng.uniform(-2, 2, (B, per ** l, per, 2)) * 16) / 16 * (3.0 if cls == "clip" else 1.0) for l in range(L)]
        shape = _compose(tabs, per, L)
        plan = [plans[(v + b) % len(plans)] for b in range(B)]
        case = dict(pos=_f32(_arrange(rng, shape, per, L, plan)), shape=_f32(shape), ivel=_f32(_ivel(rng, B)))
        info = {}
        model(observations(case), per, info=info)
        for b in range(B):
            # envs are taken in variant order, so that a short case set still holds one env of each of its first variants
            if cls in ("rank", "clip") and info["formed"][b]:
                continue
            if info["margin"][b] >= floor and (v + b) % len(plans) == len(kept) % len(plans) and len(kept) < pool:
                kept.append({k: x[b] for k, x in case.items()})
                infos.append({k: x[b] for k, x in info.items()})
        v += B
        if len(kept) >= pool:
            break
    assert len(kept) >= pool, (cls, per, L, len(kept))
    if cls == "rank":
        feats, have, order = ("fallback", "rank1", "rank2"), np.zeros(3), []
        for _ in range(n):                                  # greedy: the env that adds most to the rarest of the three so far
            gain = lambda e: sum(min(infos[e][f], 2) / (1.0 + have[j]) for j, f in enumerate(feats))
            e = max((e for e in range(pool) if e not in order), key=lambda e: (gain(e), -e))
            order.append(e)
            have += [infos[e][f] for f in feats]
        kept = [kept[e] for e in sorted(order[:n])]
    return {k: np.stack([c[k] for c in kept]) for k in kept[0]}


def _ties(per, L, seed):
    """Every sub-group's offsets (positions and shape alike) are multiples of 1/4 that sum to zero inside their group: sub-group
    centroids are then sums of their ancestors' offsets, on the same grid at every level, and exact ties abound.  From a pool,
    the envs are kept where everything compared is exact in fp32 and a tie rule decides the action (the tie mutants move it)."""
    N, n = per ** L, _n_envs(per ** L)
    rng = np.random.RandomState(seed)
    kept = {m: [] for m in TIE_MUTANTS}
    quota = 8 if N <= 64 else 3                                # envs per tie rule: at one level an env may hold a single such row
    for _ in range(40):
        B = 32 if N <= 64 else 8

        def tabs():
            t = [rng.randint(-3, 4, (B, per ** l, per, 2)) / 4.0 for l in range(L)]
            for x in t:
                x[:, :, -1] = -x[:, :, :-1].sum(2)
                for b in range(B):                             # the zero-sum entry goes anywhere, not always last
                    x[b] = x[b][:, rng.permutation(per)]
            return _compose(t, per, L)
        case = dict(pos=tabs() + rng.randint(-4, 5, (B, 1, 2)) / 4.0, shape=tabs(), ivel=np.round(_ivel(rng, B) * 8) / 8)
        obs = observations(case)
        info = {}
        base = model(obs, per, info=info)
        for m in TIE_MUTANTS:
            moved = (np.abs(model(obs, per, m) - base).max(-1) > 10 * bound(base)[:, None]).sum(1)
            for b in np.argsort(-moved, kind="stable"):
                if info["exact"][b] and moved[b] > 0 and len(kept[m]) < quota:
                    kept[m].append({k: x[b] for k, x in case.items()})
        if all(len(v) >= quota for v in kept.values()):
            break
    flat = [c for m in TIE_MUTANTS for c in kept[m]]
    assert len(flat) >= len(TIE_MUTANTS), (per, L, {m: len(v) for m, v in kept.items()})
    return {k: np.stack([c[k] for c in flat]) for k in flat[0]}


@functools.lru_cache(maxsize=None)
def cases(per, L):
    """{class: dict(pos, shape, ivel)} for the hierarchy; deterministic."""
    out = {}
    for n, cls in enumerate(CLASSES):
        seed = 1000 * per + 100 * L + n
        if cls == "ties":
            if per in TIE_PER:
                out[cls] = _ties(per, L, seed)
        else:
            out[cls] = _designed(cls, per, L, seed)
    return out


@functools.lru_cache(maxsize=None)
def stacked(per, L):
    """All classes of the hierarchy as one batch: (case dict, fp32-valued observations [B, N, 6N], {class: slice})."""
    cs = cases(per, L)
    case = {k: np.concatenate([cs[c][k] for c in cs]) for k in ("pos", "shape", "ivel")}
    sl, at = {}, 0
    for c in cs:
        sl[c] = slice(at, at + len(cs[c]["pos"]))
        at = sl[c].stop
    return case, observations(case), sl


@functools.lru_cache(maxsize=None)
def reference(per, L):
    """The fp64 oracle's actions [B, N, 2] on `stacked(per, L)`, computed once and shared."""
    obs = stacked(per, L)[1]
    want = np.stack([np.array(O.get_action_bfs(ezpolicy_stable, list(o), per, strict=False)) for o in obs])
    want.setflags(write=False)
    return want
