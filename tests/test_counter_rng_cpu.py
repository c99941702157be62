"""The NumPy reference of the device counter RNG (tests/counter_rng.py) checked on its own, and the inputs of
tests/test_gpu_counter_rng.py checked for what they can tell apart.  No GPU.

Discrimination.  A GPU comparison with the reference is worth what the reference's mutants differ by AT THE COMPARED VALUES:
a dropped seed high word is invisible at a seed below 2^32, a centring by the lane-group width at N = 4.  Every mutant below is
built from the reference (`counter_rng.Variant`) at the exact (seed, base, offset, K, sizes) the GPU tests use, over the values
in which the mutation can show at all - named per mutant - and must differ from the true reference in >= 99 % of them: exact
draws by any amount (a 24-bit value repeats by chance once in 2^24), ideal shapes by more than the shape bound, Gaussian draws
by more than ten times the per-draw bound.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "gym-formation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import formation_oracle as O   # noqa: E402
from tests import counter_rng as R         # noqa: E402
from tests.counter_rng import BASE, K, OFFSETS, SEED, Variant  # noqa: E402


# ---- the reference itself ----
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32-10."""
    got = R.philox(*ctr, key[0] | (key[1] << 32))
    assert tuple(int(x) for x in got) == want
    assert tuple(int(x) for x in R._philox(*ctr, key[0] | (key[1] << 32))) == want
    nine = R.philox(*ctr, key[0] | (key[1] << 32), rounds=9)
    assert tuple(int(x) for x in nine) != want


def test_philox_is_elementwise():
    rs = np.random.RandomState(0)
    c = rs.randint(0, 2 ** 32, (4, 7), dtype=np.uint64)
    seed = 0x0123456789ABCDEF
    got = R.philox(*c, seed)
    for j in range(7):
        one = R.philox(*[int(x) for x in c[:, j]], seed)
        assert [int(w[j]) for w in got] == [int(x) for x in one]


def test_u_pm1_is_exact_in_fp32_over_all_inputs():
    """u_pm1 looks at the upper 24 bits only: all 2^24 of them.  The fp32 evaluation as the device writes it - (float)(x >> 8)
    times 2^-23, minus 1, as two roundings or as one fma - equals the fp64 value, which lies in [-1, 1) and reaches -1."""
    m = np.arange(2 ** 24, dtype=np.uint64)
    ref = R.u_pm1(m << np.uint64(8))
    assert np.array_equal(R.u_pm1((m << np.uint64(8)) | np.uint64(0xFF)), ref), "the low 8 bits must not matter"
    f = m.astype(np.float32)
    assert np.array_equal(f.astype(np.float64), m.astype(np.float64))
    two_roundings = f * np.float32(2.0 / 16777216.0) - np.float32(1.0)
    assert two_roundings.dtype == np.float32 and np.array_equal(two_roundings.astype(np.float64), ref)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)                 # an fma's single rounding: none either
    assert ref.min() == -1.0 and ref.max() == 1.0 - 2.0 ** -23 and ref[0] == -1.0


def test_gauss_pair_is_box_muller():
    c0 = np.array([0, 0xFFFFFFFF, 0x80000000, 0x12345678], dtype=np.uint64)
    c1 = np.array([0, 0x40000000, 0x80000000, 0xC0000000], dtype=np.uint64)
    g = R.gauss_pair(c0, c1)
    r = np.sqrt(-2.0 * np.log(((c0 >> np.uint64(8)).astype(np.float64) + 1) / 2 ** 24))
    assert np.allclose(np.hypot(g[:, 0], g[:, 1]), r, rtol=1e-15) and r[1] == 0.0 and np.isfinite(r).all()
    assert abs(r[0] - np.sqrt(2 * 24 * np.log(2.0))) < 1e-12                              # the largest radius: u = 2^-24
    assert abs(g[1:, :].sum()) < 10 and g[0, 1] == 0.0 and g[0, 0] == r[0]                # angle 0
    tau32 = float(np.float32(6.2831853))
    assert np.allclose(np.arctan2(g[3, 1], g[3, 0]) % (2 * np.pi), 0.75 * tau32, atol=1e-12)
    assert R.gauss_bound(2.7) < 2e-6 < R.gauss_bound(2.8)


def test_stream_codes_are_pairwise_disjoint():
    """No two consumers of one scenario family can draw the same block: the code sets over i, l, k < 1024 and q < 2^16
    are pairwise disjoint (hd_reset and scn_agent are the same code by design: a world is one scenario or the other)."""
    i = np.arange(1024, dtype=np.uint64)
    q = np.arange(2 ** 16, dtype=np.uint64)
    sets = {
        "agent": i,
        "hd_ivel": np.array([R.STREAM_CODES["hd_ivel"]()], dtype=np.uint64),
        "scn_landmark": np.array([R.STREAM_CODES["scn_landmark"](int(x)) for x in i], dtype=np.uint64),
        "scn_obstacle": np.array([R.STREAM_CODES["scn_obstacle"](int(x)) for x in i], dtype=np.uint64),
        "motor_noise": np.array([R.STREAM_CODES["motor_noise"](int(x)) for x in i], dtype=np.uint64),
        "actor_noise": np.array([R.STREAM_CODES["actor_noise"](int(x)) for x in i], dtype=np.uint64),
        "comm_noise": ((i[None, :] | np.uint64(0x40000000) | (q[:, None] << np.uint64(12))) ^ np.uint64(0x80000000)).ravel(),
    }
    assert R.STREAM_CODES["hd_reset"] is R.STREAM_CODES["scn_agent"]
    assert [R.STREAM_CODES["hd_reset"](int(x)) for x in i[:5]] == [0, 1, 2, 3, 4]
    for a in (0, 1, 5, 1023):                                                             # the vectorised comm set is the function's
        for b in (0, 1, 7, 65535):
            assert R.STREAM_CODES["comm_noise"](a, b) == int(sets["comm_noise"][b * 1024 + a])
    # the comm set is built q-major with i ascending: strictly increasing means distinct, and lets the small sets be searched in it
    comm = sets.pop("comm_noise")
    assert bool((np.diff(comm.astype(np.int64)) > 0).all()) and int(comm.max()) < 2 ** 32
    names = sorted(sets)
    for s in sets.values():
        assert len(np.unique(s)) == len(s) and int(s.max()) < 2 ** 32
    for x in range(len(names)):
        at = np.minimum(np.searchsorted(comm, sets[names[x]]), len(comm) - 1)
        assert not (comm[at] == sets[names[x]]).any(), (names[x], "comm_noise")
        for y in range(x + 1, len(names)):
            assert not np.intersect1d(sets[names[x]], sets[names[y]]).size, (names[x], names[y])
    assert R.IVEL_CODE not in set(int(x) for x in sets["motor_noise"])    # 0xFFFFFFFF = i ^ 0x80000000 only at i = 0x7FFFFFFF > 1023
    assert 0xFFFFFFFF ^ 0x80000000 == 0x7FFFFFFF and 0x7FFFFFFF >= 1024


def test_centring_formula_is_the_oracles():
    """reset_hd (MT19937 draws) and hd_reset (Philox draws) centre alike: shape = raw - mean over the N agents, rows sum to 0."""
    for N in (3, 27, 200):
        st = O.reset_hd(1 + 1000 * np.arange(4), N)
        assert np.abs(st["ideal_shape"].sum(1)).max() <= 1e-15 * N
        ref = R.hd_reset(SEED, BASE, 4, N, 5)
        assert np.abs(ref["shape"].sum(1)).max() <= 1e-15 * N
        assert np.array_equal(ref["shape"], ref["raw"] - ref["raw"].sum(1, keepdims=True) / N)
        assert np.allclose(ref["shape"], ref["raw"] - ref["raw"].mean(1, keepdims=True), rtol=0, atol=1e-15)
        _, raw, _ = O.reset_draws(1, N)
        assert np.allclose(st["ideal_shape"][0], raw - raw.sum(0) / N, rtol=0, atol=1e-15)


def test_reference_shapes_ranges_and_keys():
    N, B, L, M = 5, 7, 4, 3
    h = R.hd_reset(SEED, BASE, B, N, 5)
    assert h["pos"].shape == (B, N, 2) and h["raw"].shape == (B, N, 2) and h["shape"].shape == (B, N, 2) and h["ivel"].shape == (B, 2)
    s = R.scn_reset(SEED, BASE, B, N, 5, L, M)
    assert s["pos"].shape == (B, N, 2) and s["lm"].shape == (B, L, 2) and s["opos"].shape == (B, M, 2)
    assert np.array_equal(s["pos"], h["pos"])                                             # the same code, the same block
    edges = np.linspace(-1.8, 1.8, M + 1)
    for k in range(M):
        assert (s["opos"][:, k, 0] >= edges[k]).all() and (s["opos"][:, k, 0] <= edges[k + 1]).all()
    assert (s["opos"][..., 1] >= 2.0).all() and (s["opos"][..., 1] < 2.5).all()
    assert R.scn_reset(SEED, BASE, B, N, 5, L, 0)["opos"].shape == (B, 0, 2)
    # env b of a batch at base 3 is env b + 3 of the batch at base 0; a launch's steps are consecutive offsets
    assert np.array_equal(R.hd_reset(SEED, 0, B + 3, N, 5)["pos"][3:], h["pos"])
    assert R.launch_offsets(2 ** 32 - 2, 4) == [2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]
    assert R.launch_offsets(2 ** 64 - 1, 2) == [2 ** 64 - 1, 0]
    c2 = R.comm_noise(SEED, BASE, B, N, 5, 2)
    for d in R.COMM_DIMS:
        c = R.comm_noise(SEED, BASE, B, N, 5, d)
        assert c.shape == (B, N, d) and np.array_equal(c[..., :min(d, 2)], c2[..., :min(d, 2)])
    assert np.array_equal(R._eps_ref(SEED, B, N, 5, base=BASE), R.actor_noise(SEED, BASE, B, N, 5))
    assert [R.lane_group(n) for n, _ in R.HD_RESET_SIZES] == [4, 4, 8, 16, 32, 32, 64, 128, 128, 256, 256, 1024]


# ---- discrimination: the mutants at the GPU tests' inputs ----
def _frac(a, b, more_than=0.0):
    d = np.abs(np.asarray(a) - np.asarray(b)) > more_than
    return d.mean(), d.size


def _gauss_gap(ref):
    r = np.sqrt((ref * ref).sum(-1, keepdims=True))
    return 10.0 * R.gauss_bound(r)


def _consumers(v, offsets, only=None):
    """name -> [(true values, mutant values, threshold)] of every consumer (or those named) at the GPU tests' sizes and the
    given (true, mutant) offsets."""
    out = {}

    def add(name, fn, thr=None):
        if only and name not in only:
            return
        for off_true, off_mut in offsets:
            t, m = fn(R.TRUE, off_true), fn(v, off_mut)
            out.setdefault(name, []).append((t, m, 0.0 if thr is None else thr(t)))
    for N, B in R.HD_RESET_SIZES:
        add("hd_pos", lambda w, o: R.hd_reset(SEED, BASE, B, N, o, w)["pos"])
        add("hd_raw", lambda w, o: R.hd_reset(SEED, BASE, B, N, o, w)["raw"])
        add("hd_ivel", lambda w, o: R.hd_reset(SEED, BASE, B, N, o, w)["ivel"])
    for N, B, L, M in SCN_SIZES:
        add("scn_pos", lambda w, o: R.scn_reset(SEED, BASE, B, N, o, L, M, w)["pos"])
        add("scn_lm", lambda w, o: R.scn_reset(SEED, BASE, B, N, o, L, M, w)["lm"])
        if M:
            add("scn_opos", lambda w, o: R.scn_reset(SEED, BASE, B, N, o, L, M, w)["opos"], lambda t: 4 * 2.0 ** -23 * 2.5)
    for N, B in R.MOTOR_SIZES:
        add("motor", lambda w, o: R.motor_noise(SEED, BASE, B, N, o, w), _gauss_gap)
        add("actor", lambda w, o: R.actor_noise(SEED, BASE, B, N, o, w), _gauss_gap)
    for d in R.COMM_DIMS:
        add("comm", lambda w, o: R.comm_noise(SEED, BASE, R.COMM_SIZE[1], R.COMM_SIZE[0], o, d, w), _gauss_gap)
    return out


SCN_SIZES = [c[2:] for c in R.SCN_CASES]          # (N, B, L, M)
SAME = [(o, o) for o in OFFSETS]


def _assert_all_differ(v, offsets, what, only=None):
    n = 0
    for name, rows in _consumers(v, offsets, only).items():
        for t, m, thr in rows:
            frac, size = _frac(t, m, thr)
            assert frac >= 0.99, "%s: %s differs in %.4f of %d values" % (what, name, frac, size)
            n += 1
    assert n, what


def test_nine_rounds_differ_everywhere():
    _assert_all_differ(Variant(rounds=9), SAME, "9 rounds")


def test_a_dropped_seed_high_word_differs_everywhere():
    assert SEED >> 32 and SEED & 0xFFFFFFFF
    _assert_all_differ(Variant(seed_mask=0xFFFFFFFF), SAME, "seed high word zeroed")


def test_a_dropped_offset_high_word_differs_at_the_high_offsets():
    """Visible where the offset's high word is set: the by-value offset 2^32 + 7, and steps 2 and 3 of the launch at 2^32 - 2
    (a sum that does not carry).  At offset 5 the mutant IS the reference - which is why the GPU cases do not stop there."""
    v = Variant(offset_mask=0xFFFFFFFF)
    high = [(o, o) for o in (OFFSETS[1],) + tuple(R.launch_offsets(OFFSETS[2], K)[2:])]
    assert all(o >> 32 for o, _ in high) and not any(o >> 32 for o in R.launch_offsets(OFFSETS[2], K)[:2])
    _assert_all_differ(v, high, "offset high word zeroed")
    assert np.array_equal(R.hd_reset(SEED, BASE, 4, 9, OFFSETS[0], v)["pos"], R.hd_reset(SEED, BASE, 4, 9, OFFSETS[0])["pos"])


def test_an_offset_that_does_not_advance_differs_from_step_one_on():
    """Step k >= 1 of every K = 4 launch (the GPU tests compare envs whose episode ends at k = 2 and k = K - 1, and every step
    of the motor noise); at k = 0 the mutant is the reference."""
    v = Variant(advance=False)
    for rbase in OFFSETS:
        true, mut = R.launch_offsets(rbase, K), R.launch_offsets(rbase, K, v)
        assert true[0] == mut[0] and len(set(true)) == K
        _assert_all_differ(R.TRUE, list(zip(true[1:], mut[1:])), "offset not advanced")


def test_a_dropped_env_index_base_differs_everywhere():
    assert BASE != 0
    _assert_all_differ(Variant(use_base=False), SAME, "env_index_base dropped")


def test_ideal_velocity_from_agent_zero_differs():
    _assert_all_differ(Variant(ivel_from_agent0=True), SAME, "ivel from agent 0's block", only=("hd_ivel",))


def test_shape_from_the_position_words_differs():
    _assert_all_differ(Variant(shape_words=(0, 1)), SAME, "shape from c0, c1", only=("hd_raw",))
    for N, B in R.HD_RESET_SIZES:                                # ... and by more than the bound the shape is held to
        t, m = R.hd_reset(SEED, BASE, B, N, 5), R.hd_reset(SEED, BASE, B, N, 5, Variant(shape_words=(0, 1)))
        frac, size = _frac(t["shape"], m["shape"], R.shape_bound(t["raw"], N))
        assert frac >= 0.99, (N, frac)


def test_centring_by_the_lane_group_differs_beyond_the_shape_bound():
    """Dividing the sum by G instead of N moves every component of an env by sum (1 / N - 1 / G).  At N = 4 and N = 1024 G is
    N and the mutant is the reference; at every other size of the GPU tests it must exceed the bound the shape is held to in
    >= 99 % of the values (which is what a moment test at 0.02 could not see at N = 27: the shift there is ~0.01)."""
    seen = 0
    for N, B in R.HD_RESET_SIZES:
        G = R.lane_group(N)
        for off in OFFSETS:
            t = R.hd_reset(SEED, BASE, B, N, off)
            m = R.hd_reset(SEED, BASE, B, N, off, Variant(centre_by=G))
            if G == N:
                assert N in (4, 1024) and np.array_equal(t["shape"], m["shape"])
                continue
            frac, size = _frac(t["shape"], m["shape"], R.shape_bound(t["raw"], N))
            assert frac >= 0.99, "N = %d: centring by G = %d differs beyond the bound in %.4f of %d values" % (N, G, frac, size)
            seen += 1
    assert seen == 3 * (len(R.HD_RESET_SIZES) - 2)


def _as(f):
    """A consumer's code function behind any consumer's call signature (agent / landmark / obstacle index [, pair])."""
    return lambda i=0, *more: f(i)


CONSUMERS = sorted(R.STREAM_CODES)


@pytest.mark.parametrize("victim", CONSUMERS)
@pytest.mark.parametrize("donor", CONSUMERS)
def test_a_swapped_stream_code_differs(victim, donor):
    """`victim` drawing with `donor`'s code.  (hd_reset and scn_agent share one code by design: no mutant.  A comm pair q > 0
    that takes another consumer's code loses its q: every consumer of the victim is compared, pair 0 included.)"""
    if victim == donor or R.STREAM_CODES[victim] is R.STREAM_CODES[donor]:
        assert victim == donor or {victim, donor} == {"hd_reset", "scn_agent"}
        return
    touched = {"hd_reset": ("hd_pos", "hd_raw"), "hd_ivel": ("hd_ivel",), "scn_agent": ("scn_pos",), "scn_landmark": ("scn_lm",),
               "scn_obstacle": ("scn_opos",), "motor_noise": ("motor",), "comm_noise": ("comm",), "actor_noise": ("actor",)}[victim]
    _assert_all_differ(Variant(codes={victim: _as(R.STREAM_CODES[donor])}), SAME, "%s with %s's code" % (victim, donor), only=touched)
