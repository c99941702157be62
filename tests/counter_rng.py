"""The one NumPy reference of the device counter RNG (csrc/fg_common.hpp: philox4x32, u_pm1, motor_noise): every stream the
kernels draw from, as plain functions of (seed, env_index_base, B, N, offset) in uint64 / fp64 arithmetic.  A plain module:
no fixtures, nothing registered with pytest.  tests/test_counter_rng_cpu.py checks this module against the published
Random123 vectors and shows that its mutants (`Variant`) are told apart at the GPU tests' inputs; tests/test_gpu_counter_rng.py
and tests/test_gpu_actor_sample.py hold the kernels to it.

The contract.  One Philox4x32-10 block per draw: key = (seed low word, seed high word), counter = (global env index =
env_index_base + b, entity code, offset low word, offset high word); step k of a K-step launch draws at offset rbase + k
(64-bit sum, rbase = FgParams.rng_offset + *rng_offset_dev).  Entity codes (counter word 1): STREAM_CODES below.
Uniform draws are u_pm1(word) = (word >> 8) 2^-23 - 1, exact in fp32 (24-bit integer, one exact scaling, one exact
subtraction: the result is a multiple of 2^-23 in [-1, 1)), so device positions, landmarks and ideal velocities equal this
reference bit for bit.  Gaussian draws are Box-Muller of words 0 and 1.

Gaussian per-draw bound.  eps = (r cos a, r sin a), r = sqrt(-2 ln u), u = ((c0 >> 8) + 1) / 2^24, a = 6.2831853f (c1 >> 8) / 2^24.
u is exact in fp32 and a carries one rounding (2^-24 relative), so the error is that of the fp32 transcendentals.  __logf is
v_log_f32 (log2, ~1 ulp) times ln 2 (0.5 ulp): ln u to ~2^-22 relative; the square root halves that and adds 0.5 ulp: r to
~2.5e-7 relative.  __cosf / __sinf scale a by 1 / 2 pi (0.5 ulp of a revolution < 1) and take v_cos_f32 / v_sin_f32 (~2^-22
absolute): cos a, sin a to ~4e-7 absolute.  Per component
    |eps - eps64| <= r (2.5e-7 |cos a| + 4e-7) + 0.5 ulp(eps) <= 7e-7 r + 1e-7        (`gauss_bound(r)`),
which is below 2e-6 for r <= 2.7 (97 % of the draws) and grows in the tail.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
MASK64 = (1 << 64) - 1
IVEL_CODE = 0xFFFFFFFF


# ---- the stream codes (counter word 1), one function per consumer ----
def _hd_agent(i):
    return i


def _hd_ivel(_=None):
    return IVEL_CODE


def _scn_landmark(l):
    return 0x10000000 | l


def _scn_obstacle(k):
    return 0x20000000 | k


def _motor(i):
    return i ^ 0x80000000


def _comm(i, q=0):
    return (i | 0x40000000 | (q << 12)) ^ 0x80000000


def _actor(i):
    return (i | 0x20000000) ^ 0x80000000


STREAM_CODES = {"hd_reset": _hd_agent, "hd_ivel": _hd_ivel, "scn_agent": _hd_agent, "scn_landmark": _scn_landmark,
                "scn_obstacle": _scn_obstacle, "motor_noise": _motor, "comm_noise": _comm, "actor_noise": _actor}


class Variant(object):
    """What a reference computes beyond its arguments.  The defaults are the device contract; test_counter_rng_cpu.py
    overrides one field at a time to build the mutants the GPU tests must be able to tell from it."""
    rounds = 10
    seed_mask = MASK64                 # 0xFFFFFFFF: the seed's high word dropped
    offset_mask = MASK64               # 0xFFFFFFFF: the offset's high word dropped / not carried into
    advance = True                     # step k of a launch draws at rbase + k
    use_base = True                    # env_index_base added to the env index
    ivel_from_agent0 = False           # the ideal velocity from agent 0's block instead of its own
    shape_words = (2, 3)               # the raw ideal shape's words of the agent's block
    centre_by = None                   # divisor of the shape centring (None: N)

    def __init__(self, **kw):
        self.codes = dict(STREAM_CODES)
        for k, v in kw.items():
            if k == "codes":
                self.codes.update(v)
            else:
                assert hasattr(Variant, k), k
                setattr(self, k, v)


TRUE = Variant()


def philox(c0, c1, c2, c3, seed, rounds=10):
    """Philox4x32 (Salmon et al. 2011) of the counter words (arrays or scalars), both key words from the 64-bit seed."""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in (c0, c1, c2, c3)]
    seed = int(seed)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(rounds):
        m0 = np.uint64(0xD2511F53) * c[0]
        m1 = np.uint64(0xCD9E8D57) * c[2]
        n0 = (m1 >> np.uint64(32)) ^ c[1] ^ k0
        n2 = (m0 >> np.uint64(32)) ^ c[3] ^ k1
        c = [n0 & M32, m1 & M32, n2 & M32, m0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def u_pm1(word):
    """U[-1, 1) of a 32-bit word, fp64 (exactly representable in fp32)."""
    return (np.asarray(word, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) * 2.0 ** -23 - 1.0


def gauss_pair(c0, c1):
    """fp64 Box-Muller of two words as motor_noise computes it: [..., 2]; 6.2831853f is the device's fp32 constant."""
    u = ((np.asarray(c0, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
    a = float(np.float32(6.2831853)) * ((np.asarray(c1, dtype=np.uint64) >> np.uint64(8)).astype(np.float64) / 16777216.0)
    r = np.sqrt(-2.0 * np.log(u))
    return np.stack([r * np.cos(a), r * np.sin(a)], -1)


def gauss_bound(r):
    """The per-component bound of an fp32 device draw of radius r against gauss_pair (module docstring)."""
    return 7e-7 * np.asarray(r, dtype=np.float64) + 1e-7


def launch_offsets(rbase, K, v=TRUE):
    """The offsets of the K steps of a launch whose base offset is rbase (64-bit wrap-around sum)."""
    return [((int(rbase) + (k if v.advance else 0)) & MASK64) for k in range(K)]


def blocks(seed, env_index_base, B, codes, offset, v=TRUE):
    """The four Philox words, each [B, len(codes)], of envs env_index_base .. + B and the entity codes `codes`."""
    g = np.arange(B, dtype=np.uint64)[:, None] + np.uint64(env_index_base if v.use_base else 0)
    codes = np.atleast_1d(np.asarray(codes, dtype=np.uint64))[None, :]
    shape = (B, codes.shape[1])
    off = int(offset) & v.offset_mask
    return philox(np.broadcast_to(g, shape), np.broadcast_to(codes, shape), np.full(shape, off & 0xFFFFFFFF, np.uint64),
                  np.full(shape, off >> 32, np.uint64), int(seed) & v.seed_mask, v.rounds)


def _codes(v, name, n, *more):
    return [v.codes[name](i, *more) for i in range(n)]


def hd_reset(seed, env_index_base, B, N, offset, v=TRUE):
    """formation_hd_env's device reset: pos [B,N,2], raw [B,N,2] (the landmarks before centring), shape = raw - raw.sum(1) / N
    [B,N,2] in fp64, ivel [B,2]."""
    c = blocks(seed, env_index_base, B, _codes(v, "hd_reset", N), offset, v)
    pos = np.stack([u_pm1(c[0]), u_pm1(c[1])], -1)
    raw = np.stack([u_pm1(c[v.shape_words[0]]), u_pm1(c[v.shape_words[1]])], -1)
    shape = raw - raw.sum(1, keepdims=True) / float(v.centre_by or N)
    if v.ivel_from_agent0:
        ivel = pos[:, 0].copy()
    else:
        ci = blocks(seed, env_index_base, B, [v.codes["hd_ivel"]()], offset, v)
        ivel = np.stack([u_pm1(ci[0][:, 0]), u_pm1(ci[1][:, 0])], -1)
    return dict(pos=pos, raw=raw, shape=shape, ivel=ivel)


def scn_reset(seed, env_index_base, B, N, offset, L, M, v=TRUE):
    """The landmark scenarios' device reset: pos [B,N,2], lm [B,L,2], opos [B,M,2] - obstacle k uniform in
    [s_k, s_k+1] x [2.0, 2.5], s = -1.8 + 3.6 k / M, as scn_fresh_obstacle computes it but in fp64 from the fp32-exact draws."""
    def pm1(name, n):
        c = blocks(seed, env_index_base, B, _codes(v, name, n), offset, v)
        return np.stack([u_pm1(c[0]), u_pm1(c[1])], -1)
    out = dict(pos=pm1("scn_agent", N), lm=pm1("scn_landmark", L), opos=np.zeros((B, M, 2)))
    if M:
        r = pm1("scn_obstacle", M)
        k = np.arange(M, dtype=np.float64)
        lo, hi = -1.8 + 3.6 * k / M, -1.8 + 3.6 * (k + 1) / M
        out["opos"] = np.stack([lo + (hi - lo) * (0.5 * r[..., 0] + 0.5), 2.0 + 0.5 * (0.5 * r[..., 1] + 0.5)], -1)
    return out


def _gauss(seed, env_index_base, B, codes, offset, v):
    c = blocks(seed, env_index_base, B, codes, offset, v)
    return gauss_pair(c[0], c[1])


def motor_noise(seed, env_index_base, B, N, offset, v=TRUE):
    """The unit motor-noise draws of one step: [B,N,2]."""
    return _gauss(seed, env_index_base, B, _codes(v, "motor_noise", N), offset, v)


def comm_noise(seed, env_index_base, B, N, offset, dim_c, v=TRUE):
    """The unit communication-noise draws of one update: [B,N,dim_c]; pair q (components 2q, 2q + 1) has its own code, the
    second half of an odd dim_c's last pair is not used."""
    pairs = (dim_c + 1) // 2
    n = np.concatenate([_gauss(seed, env_index_base, B, _codes(v, "comm_noise", N, q), offset, v) for q in range(pairs)], -1)
    return n[..., :dim_c]


def actor_noise(seed, env_index_base, B, N, offset, v=TRUE):
    """The unit exploration draws of one step of the fused Gaussian actor: [B,N,2]."""
    return _gauss(seed, env_index_base, B, _codes(v, "actor_noise", N), offset, v)


# the names tests/test_gpu_actor_sample.py has always used
_philox = philox


def _eps_ref(seed, Bn, N, offset, base=0):
    return actor_noise(seed, base, Bn, N, offset)


# ---- the inputs of tests/test_gpu_counter_rng.py (test_counter_rng_cpu.py shows that they tell the mutants apart) ----
SEED = 0x9E3779B97F4A7C15                   # both key words non-zero
BASE = 3                                    # env_index_base
K = 4
OFFSETS = (5, 2 ** 32 + 7, 2 ** 32 - 2)     # low; high word set; steps 2 and 3 of a K = 4 launch carry into the high word
HD_RESET_SIZES = [(3, 70), (4, 65), (5, 33), (9, 37), (17, 9), (27, 13), (33, 6), (65, 4), (81, 3), (200, 2), (243, 2), (1024, 1)]
HD_LAUNCH_SIZES = [(3, 70), (9, 37), (27, 13), (81, 3), (243, 2)]
HD_OPTION_SIZES = [(17, 9), (200, 2)]
# (scenario, oracle kind, N, B, L, M): the four landmark scenarios at their own agent counts (the one-env-per-lane kernels'
# shapes; 3 obstacles), and 70 agents + 3 obstacles - one env per workgroup of the run-time-count kernel
SCN_CASES = [("basic_formation_env", None, 3, 37, 3, 0), ("formation_hd_partial_env", "partial", 5, 37, 5, 0),
             ("formation_hd_partial_range_env", "range", 4, 37, 4, 0), ("formation_hd_obs_env", "obstacle", 4, 37, 4, 3),
             ("formation_hd_obs_env", "obstacle", 70, 9, 4, 3)]
MOTOR_SIZES = [(5, 33), (9, 37), (65, 4)]
COMM_SIZE = (5, 33)
COMM_DIMS = (1, 2, 3, 5)


def lane_group(N):
    """Lanes that share one env's reductions: the power of two >= N, at least 4, at least 128 above 64 agents (one env per
    workgroup there)."""
    g = 4
    while g < N:
        g <<= 1
    return g if N <= 64 else max(g, 128)


def shape_bound(raw, N):
    """Per env and component [B,1,2]: the bound of the device's fp32 ideal shape against hd_reset's fp64 `shape`.
    The device sums the N raw values (multiples of 2^-23 below 1) in fp32 over a tree of lane_group(N) - 1 additions (those with a
    padded lane's zero are exact), multiplies by the rounded 1 / N and subtracts from the raw value in one fma.  With
    S = sum_i |raw_i| every partial sum is at most S, so the sum is off by at most (additions that round) 2^-24 S; the rounded
    1 / N adds 2^-24 S / N, which the padded additions (G > N) or the exact 1 / N (G == N: a power of two) make room for; the
    fma rounds once, by at most 2^-24 below 2:
        |shape - shape64| <= (G - 1) 2^-24 S / N + 2^-24.
    While S < 2 every partial sum is a multiple of 2^-23 below 2, hence exact, |shape| < 1 rounds by at most 2^-25 and the
    rounded 1 / 3 adds at most 2^-25 2 / 3: the bare 2^-24 holds (`S < 2` rows of the N = 3 and N = 4 cases)."""
    S = np.abs(raw).sum(1, keepdims=True)
    return (lane_group(N) - 1) * 2.0 ** -24 * S / N + 2.0 ** -24
