// fg_planner_kernels.hpp - A sampling planner's candidates without a candidate tensor: actions drawn where they are used
// (fg_rollout_hd_returns_sampled), the same actions as a tensor (fg_plan_candidates) and MPPI's weighted average of them
// (fg_plan_mppi_update).  Part of libformation_hip (gfx950); included by formation_hip.hip, one translation unit.  fp32 only:
// the sampled launch is tied, bit for bit, to returns_kernel, which the fp64 parity build checks.
#ifndef FG_PLANNER_KERNELS_HPP_
#define FG_PLANNER_KERNELS_HPP_

#include "fg_common.hpp"
#include "fg_returns_kernel.hpp"

namespace fg {

// ---------------------------------------------------------------------------
// One spelling of a candidate action: u = clamp(mean + sigma eps), eps from the planner's own counter stream.
// ---------------------------------------------------------------------------
constexpr int FG_PLAN_MAX_N = 1 << 12;         // agent index: bits 0 .. 11 of the stream code
constexpr int FG_PLAN_MAX_C = 1 << 17;         // candidate index: bits 12 .. 28

// The unit normal pair of candidate c, agent i of global env g at counter offset `offset`: motor_noise's Box-Muller of the
// Philox block {g, 0x40000000 | c << 12 | i, offset} (motor_noise flips bit 31 of the code it is given).  Top three bits of
// word 1: 010 for every i < 2^12, c < 2^17 - reset and landmarks 000, obstacles 001, Gumbel 011, motor noise 100, actor noise
// 101, communication 110, ideal velocity 111.  `offset` is the planner's own counter (step k of a call: noise_offset + k, a
// 64-bit sum), never the env's RNG offset: planning does not move the env's RNG.
FG_DEV float2 plan_eps(uint64_t seed, uint32_t g, uint32_t c, uint32_t i, uint64_t offset) {
    return motor_noise(seed, g, (0x40000000u | (c << 12) | i) ^ 0x80000000u, offset);
}

// mean + sigma eps per component, one rounded product and one rounded sum (never an fma: the tests rebuild it from the
// unit draws), then the clamp to [-clip, clip] where clip > 0
FG_DEV float2 plan_action(float2 mean, float sigma, float2 eps, float clip) {
    float2 u = make_float2(add_rn_(mean.x, mul_rn_(sigma, eps.x)), add_rn_(mean.y, mul_rn_(sigma, eps.y)));
    if (clip > 0.0f) { u.x = fminf(fmaxf(u.x, -clip), clip); u.y = fminf(fmaxf(u.y, -clip), clip); }
    return u;
}

// what a launch needs to draw: the scalars of plan_eps and plan_action
struct PlanDraw {
    uint64_t seed, noise_offset;
    uint32_t env_index_base;
    float sigma, clip;
};
FG_DEV float2 plan_draw(const PlanDraw& d, float2 mean, uint32_t b, uint32_t c, uint32_t i, uint32_t k) {
    return plan_action(mean, d.sigma, plan_eps(d.seed, b + d.env_index_base, c, i, d.noise_offset + k), d.clip);
}

// ---------------------------------------------------------------------------
// returns_sampled_kernel: returns_kernel (fg_returns_kernel.hpp: geometry, pair index, `produce`, recurrence, nsteps) with the
// action of (c, k, b, i) drawn from mean[k][b][i] instead of read from act[c][k][b][i] - the one body of both,
// fg_returns_body.inc.  It keeps the prefetch shape: the action of step k + 1 - one 8-byte load of `mean`, shared by the
// env's C candidates (neighbouring pairs: the same lines), ten Philox rounds, a log, a square root, a sine and a cosine - is
// made during step k, where returns_kernel issues its load, so that it is independent work beside the pair loops and not
// in front of them.  Past the last step nothing is drawn.
// Registers: returns_kernel's waves_per_eu(4) budget holds in every instantiation - no scratch, no spill, so none needs a
// budget of its own.  VGPRs against returns_kernel's (code object): 3 agents 68 / 68, 4: 68 / 66, 8: 84 / 82, 9: 100 / 100,
// 16: 89 / 88, 25 and 27: 82 / 80, 32: 80 / 80.  The one occupancy change is at 25 and 27 agents: 82 registers are allocated
// as 88, which is 5 resident waves per SIMD where returns_kernel's 80 give 6 (measured: profiles/planner_mppi.md).
// ---------------------------------------------------------------------------
struct ReturnsSampledArgs {
    ReturnsArgs r;             // r.act is not read
    const float* mean;         // [K][B][N][2]
    PlanDraw d;
};

template <int NC, int G, int T>
__global__ __launch_bounds__(T) FG_RETURNS_OCCUPANCY
void returns_sampled_kernel(const ReturnsSampledArgs sa) {
    const ReturnsArgs& a = sa.r;
#define FG_RETURNS_SAMPLED 1
#include "fg_returns_body.inc"
#undef FG_RETURNS_SAMPLED
}

// ---------------------------------------------------------------------------
// fg_plan_candidates: act[c][k][b][i] = plan_draw(...) for every element, any N <= 2^12; mean NULL = zeros.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void plan_candidates_kernel(const PlanDraw d, int B, int N, int K, int C,
                                                              const float2* __restrict__ mean, float2* __restrict__ act) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long row = (long long)K * B * N;                  // elements per candidate
    if (t >= row * C) return;
    const int c = (int)(t / row);
    const long long r = t - (long long)c * row;                  // (k B + b) N + i: the element of `mean`
    const int k = (int)(r / ((long long)B * N));
    const long long bi = r - (long long)k * B * N;
    const int b = (int)(bi / N), i = (int)(bi - (long long)b * N);
    const float2 m = mean ? mean[r] : make_float2(0.f, 0.f);
    act[t] = plan_draw(d, m, (uint32_t)b, (uint32_t)c, (uint32_t)i, (uint32_t)k);
}

// ---------------------------------------------------------------------------
// fg_plan_mppi_update: one thread per (k, b, i), two passes over c in ascending order in fp32 - the maximum of the row's
// returns, then the weights w_c = exp((ret_c - m) / lambda), their sum and the weighted sum of the candidates' actions, drawn
// again.  No LDS, no barrier; the second pass re-reads ret[c][b][i] (L2: the K threads of a row and both passes share it).
// new = n / s goes to mean_out[k - shift] (shift = 1: the plan moves one step on and its last step is repeated) and, for
// k = 0, to act_out.  A thread writes another thread's input row when shift = 1: mean_out must not overlap mean_in (host check).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void plan_mppi_update_kernel(const PlanDraw d, int B, int N, int K, int C, float lambda,
                                                               const float* __restrict__ ret, const float2* __restrict__ mean_in,
                                                               float2* __restrict__ mean_out, float2* __restrict__ act_out,
                                                               int shift) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long bn = (long long)B * N;
    if (t >= bn * K) return;
    const int k = (int)(t / bn);
    const long long bi = t - (long long)k * bn;
    const int b = (int)(bi / N), i = (int)(bi - (long long)b * N);
    const float* const rrow = ret + bi;                          // ret[c][b][i] = rrow[c B N]
    float m = -INFINITY;
    for (int c = 0; c < C; ++c) m = fmaxf(m, rrow[(size_t)c * bn]);
    const float2 mu = mean_in[t];
    float s = 0.f, nx = 0.f, ny = 0.f;
    // one candidate: its weight, its action drawn again, the three sums
    auto weigh = [&](int c, float& w, float2& u) {
        w = __expf((rrow[(size_t)c * bn] - m) / lambda);
        u = plan_draw(d, mu, (uint32_t)b, (uint32_t)c, (uint32_t)i, (uint32_t)k);
    };
    auto add = [&](float w, float2 u) { s += w; nx += w * u.x; ny += w * u.y; };
    // four candidates at a time: their draws are independent chains (Philox, log, sine, cosine) that overlap, and the sums
    // still take the candidates in ascending order.  With few rows (one env, thousands of candidates) the launch is this
    // loop's latency: K B N threads, C iterations each.
    int c = 0;
    for (; c + 4 <= C; c += 4) {
        float w[4];
        float2 u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) weigh(c + j, w[j], u[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) add(w[j], u[j]);
    }
    for (; c < C; ++c) {
        float w;
        float2 u;
        weigh(c, w, u);
        add(w, u);
    }
    const float2 out = make_float2(nx / s, ny / s);
    if (k >= shift) mean_out[t - (long long)shift * bn] = out;
    if (shift && k == K - 1) mean_out[t] = out;
    if (k == 0 && act_out) act_out[bi] = out;
}

// ---------------------------------------------------------------------------
// A sigma per step, env, agent and component (the cross-entropy method's second iteration): std [K][B][N][2], laid out like
// `mean`.  plan_action's roundings - one rounded product, one rounded sum per component -, so that a tensor filled with
// float32(sigma) gives the scalar entries' bits.  The caller's contract: every element of `std` is finite and >= 0 (the
// host cannot look into device memory; CEMPlanner's own std is max(sigma_min, a convex sum of such numbers)).  Stream code,
// the noise_offset + k rule, FG_PLAN_MAX_N and FG_PLAN_MAX_C: those of plan_eps.  PlanDraw's `sigma` is not read.
// ---------------------------------------------------------------------------
FG_DEV float2 plan_action_std(float2 mean, float2 sd, float2 eps, float clip) {
    float2 u = make_float2(add_rn_(mean.x, mul_rn_(sd.x, eps.x)), add_rn_(mean.y, mul_rn_(sd.y, eps.y)));
    if (clip > 0.0f) { u.x = fminf(fmaxf(u.x, -clip), clip); u.y = fminf(fmaxf(u.y, -clip), clip); }
    return u;
}
FG_DEV float2 plan_draw_std(const PlanDraw& d, float2 mean, float2 sd, uint32_t b, uint32_t c, uint32_t i, uint32_t k) {
    return plan_action_std(mean, sd, plan_eps(d.seed, b + d.env_index_base, c, i, d.noise_offset + k), d.clip);
}

// returns_sampled_std_kernel: the third use of fg_returns_body.inc (FG_RETURNS_SAMPLED == 2) - returns_sampled_kernel with
// the 8-byte load of std[k][b][i] beside that of mean[k][b][i]; geometry, prefetch shape and recurrence unchanged.
// Registers: the waves_per_eu(4) budget holds in every instantiation with no scratch and no spill.  VGPRs (code object) of
// returns_kernel / returns_sampled_kernel / this kernel: 3 agents 68 / 68 / 70, 4: 66 / 68 / 70, 8: 82 / 84 / 86,
// 9: 100 / 100 / 102, 16: 88 / 89 / 91, 25 and 27: 80 / 82 / 84, 32: 80 / 80 / 82 - two more each, the sigma pair, and no
// occupancy step crossed against returns_sampled_kernel (72, 80, 88, 96, 104 are the allocation steps in reach).
struct ReturnsSampledStdArgs {
    ReturnsArgs r;             // r.act is not read
    const float* mean;         // [K][B][N][2]
    const float* sd;           // std [K][B][N][2], finite and >= 0
    PlanDraw d;                // d.sigma is not read
};

template <int NC, int G, int T>
__global__ __launch_bounds__(T) FG_RETURNS_OCCUPANCY
void returns_sampled_std_kernel(const ReturnsSampledStdArgs sa) {
    const ReturnsArgs& a = sa.r;
#define FG_RETURNS_SAMPLED 2
#include "fg_returns_body.inc"
#undef FG_RETURNS_SAMPLED
}

// fg_plan_candidates_std: plan_candidates_kernel with the sigma tensor
__global__ __launch_bounds__(256) void plan_candidates_std_kernel(const PlanDraw d, int B, int N, int K, int C,
                                                                  const float2* __restrict__ mean, const float2* __restrict__ sd,
                                                                  float2* __restrict__ act) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long row = (long long)K * B * N;                  // elements per candidate
    if (t >= row * C) return;
    const int c = (int)(t / row);
    const long long r = t - (long long)c * row;                  // (k B + b) N + i: the element of `mean` and `std`
    const int k = (int)(r / ((long long)B * N));
    const long long bi = r - (long long)k * B * N;
    const int b = (int)(bi / N), i = (int)(bi - (long long)b * N);
    const float2 m = mean ? mean[r] : make_float2(0.f, 0.f);
    act[t] = plan_draw_std(d, m, sd[r], (uint32_t)b, (uint32_t)c, (uint32_t)i, (uint32_t)k);
}

// ---------------------------------------------------------------------------
// fg_plan_cem_update: the cross-entropy method's update, one 64-lane wave per (env, agent) row, FG_CEM_ROWS rows per
// workgroup (no workgroup barrier: a row is its wave's business).  Work per row: O(C) for the selection plus O(K E) draws.
//
// Select.  The E elites are the E largest of ret[c][b][i] under the total order of cem_key (unsigned compare of the bits,
// sign-flipped: -0 < +0, every NaN pattern has a place), equal keys ranked by ascending c.  Lane l holds the keys of
// candidates l, l + 64, ... in registers while C <= 64 KPL (KPL = 1, 8 or 64 keys per lane: C <= FG_CEM_REG_C = 4096);
// beyond (KPL = 0) every pass re-reads the row from L2 (4 C bytes strided by B N).  The E-th largest key T is built MSB
// first: 32 rounds, each the count of keys >= T | bit - a compare and a ballot per 64 keys, the count a scalar.  Then the
// keys above T are counted, and the remaining E - n places go to the keys equal to T in ascending c: a running count
// across the lane-strided iterations plus a ballot prefix within one.  Every loop is bounded by C, E, K or a constant;
// there is no loop on a device value, so no input - NaN included - can hang the kernel.
//
// Elite list.  While E <= FG_CEM_ELITE_CAP = 1024 the elites' indices are compacted, ascending, into LDS: 4 KiB per row,
// 16 KiB per workgroup, so that the 8 workgroups a CU can hold at this kernel's register count (32 waves) take 128 of its
// 160 KiB - the list never lowers the occupancy the registers allow.  elite_idx is a copy of the list, and the refit walks
// it.  Above the cap the membership predicate is evaluated in place: every refit pass walks all C candidates again,
// re-reading the row (L2) whatever KPL is.
//
// Refit.  With E <= 32 a wave serves 64 / GE steps at once (GE = E rounded up to a power of two, lane groups of GE), else
// one step per pass (GE = 64).  Per step and component: the elites' actions drawn again from (mean_in, std_in); per-lane
// partial sums over the lane's elites in ascending order, one xor-butterfly over the group (a fixed tree: two launches give
// the same bits); dm = sum(u - mean_in) / E, m = mean_in + dm; v = sum((u - m)^2) / E in a second pass (E <= 64: the drawn
// actions are still in registers; else they are drawn again).  mean_new = mean_in + alpha dm - (1 - alpha) mean_in +
// alpha m with one rounding fewer, exact when every elite equals mean_in -, std_new = max(sigma_min, (1 - alpha) std_in +
// alpha sqrt(v)).  Both go to row k - shift (shift = 1: the last step repeated), mean_new of step 0 to act_out.
// Small row counts (one env of 27 agents: 27 waves): a row's K steps were NOT split over the waves of a workgroup - see
// profiles/planner_cem.md for the measurement this rests on.
// Resources (code object): no scratch, no spill (vector or scalar); LDS 16384 bytes; VGPRs 54 at KPL 1, 8 and 0 - eight
// waves per SIMD, the 8 workgroups per CU above - and 146 at KPL 64 (the keys and their candidate indices: three).
// ---------------------------------------------------------------------------
constexpr int FG_CEM_ROWS = 4;                 // rows (waves) per workgroup
constexpr int FG_CEM_REG_C = 4096;             // keys stay in registers up to this many candidates (64 per lane)
constexpr int FG_CEM_ELITE_CAP = 1024;         // elites per row listed in LDS

FG_DEV uint32_t cem_key(float r) {
    const uint32_t bits = __float_as_uint(r);
    return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}

struct CemArgs {
    PlanDraw d;                // d.sigma is not read
    int B, N, K, C, E, shift;
    float alpha, sigma_min;
    const float* ret;          // [C][B][N]
    const float2* mean_in;     // [K][B][N]
    const float2* std_in;
    float2* mean_out;
    float2* std_out;
    float2* act_out;           // [B][N] or NULL
    int32_t* elite_idx;        // [E][B][N] or NULL
};

template <int KPL>
__global__ __launch_bounds__(64 * FG_CEM_ROWS) void plan_cem_update_kernel(const CemArgs a) {
    __shared__ int elist[FG_CEM_ROWS][FG_CEM_ELITE_CAP];
    const int l = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long bn = (long long)a.B * a.N;
    const long long row = (long long)blockIdx.x * FG_CEM_ROWS + w;
    if (row >= bn) return;                                       // (the whole wave)
    const uint32_t b = (uint32_t)(row / a.N), i = (uint32_t)(row - (long long)b * a.N);
    const float* const rrow = a.ret + row;                       // ret[c][b][i] = rrow[c B N]
    const int C = a.C, E = a.E, K = a.K;
    const uint64_t below = (1ull << l) - 1ull;                   // the lanes before this one

    const int last = (C - 1) / 64;                               // the last chunk of 64 candidates, the only one that can
    const bool tail_ok = l < C - 64 * last;                      // be short; the chunks after it hold padding only
    uint32_t keys[KPL > 0 ? KPL : 1];
    if constexpr (KPL > 0) {
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            const int c = 64 * j + l;                            // (always a load, clamped to the row: no branch per key)
            const uint32_t key = cem_key(rrow[(size_t)min(c, C - 1) * bn]);
            keys[j] = (j < last || (j == last && tail_ok)) ? key : 0u;
            if (j % 8 == 7) __builtin_amdgcn_sched_barrier(0);   // eight loads in flight, not 64 addresses in registers
        }
    }
    // f(key, c) for candidates c = l, l + 64, ... in ascending order; past C the key is 0 (c >= C tells).  scan_mem reads the
    // row again; scan takes the registers where there are any (unrolled: what it inlines is repeated KPL times, so the
    // passes that draw inside `f` go through scan_mem)
    auto scan_mem = [&](auto&& f) {
        for (int c0 = 0; c0 < C; c0 += 64) {
            const int c = c0 + l;
            f(c < C ? cem_key(rrow[(size_t)c * bn]) : 0u, c);
        }
    };
    auto scan = [&](auto&& f) {
        if constexpr (KPL > 0) {
#pragma unroll
            for (int j = 0; j < KPL; ++j) {
                f(keys[j], 64 * j + l);                              // (all KPL chunks: a bound per chunk inside the 32 rounds
                                                                     //  is hoisted out of them, one scalar register each)
                if (j % 8 == 7) __builtin_amdgcn_sched_barrier(0);   // (else 64 ballots are formed first: scalar registers spill)
            }
        } else {
            scan_mem(f);
        }
    };

    // the E-th largest key: the largest T with at least E keys >= T (a trial is >= 1, so the padding never counts)
    uint32_t T = 0u;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t trial = T | (1u << bit);
        int cnt = 0;
        scan([&](uint32_t key, int) { cnt += __popcll(__ballot(key >= trial)); });
        if (cnt >= E) T = trial;
    }
    int above = 0;
    scan([&](uint32_t key, int) { above += __popcll(__ballot(key > T)); });      // (the padding, 0, is above nothing)
    const int need = E - above;                                  // >= 1 places for the keys equal to T, lowest c first

    // f(c, selected, place) over all candidates in ascending c; `place` is the elite's rank in ascending c
    auto members = [&](auto&& over, auto&& f) {
        int seen_eq = 0, seen = 0;
        over([&](uint32_t key, int c) {
            const bool ok = c < C;                               // (T can be 0, the padding's key)
            const bool eq = ok && key == T;
            const uint64_t eqm = __ballot(eq);
            // (key >= T and not key > T: the masks of the count above would be kept for this pass, 128 scalar registers)
            const bool sel = ok && key >= T && (!eq || seen_eq + __popcll(eqm & below) < need);
            const uint64_t sm = __ballot(sel);
            f(c, sel, seen + __popcll(sm & below));
            seen_eq += __popcll(eqm);
            seen += __popcll(sm);
        });
    };

    const bool listed = E <= FG_CEM_ELITE_CAP;
    int* const list = elist[w];
    if (listed) {
        members(scan, [&](int c, bool sel, int place) { if (sel) list[place] = c; });
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (a.elite_idx)
            for (int e = l; e < E; e += 64) a.elite_idx[(size_t)e * bn + row] = list[e];
    } else if (a.elite_idx) {
        members(scan_mem, [&](int c, bool sel, int place) { if (sel) a.elite_idx[(size_t)place * bn + row] = c; });
    }

    // lane groups of GE lanes, one step each
    int GE = 64;
    if (listed)
        for (GE = 1; GE < E && GE < 64; GE <<= 1) {}
    const int KG = 64 / GE, el = l & (GE - 1), kg = l / GE;
    const float fE = (float)E;
    for (int k0 = 0; k0 < K; k0 += KG) {
        const int k = k0 + kg;
        const bool kok = k < K;
        const size_t t = (size_t)(kok ? k : 0) * bn + row;
        const float2 mu = a.mean_in[t], sd = a.std_in[t];
        auto draw = [&](int c) { return plan_draw_std(a.d, mu, sd, b, (uint32_t)c, i, (uint32_t)k); };
        auto group_sum = [&](float& x, float& y) {
            for (int o = GE >> 1; o > 0; o >>= 1) { x += __shfl_xor(x, o); y += __shfl_xor(y, o); }
        };
        // f(c) for this lane's elites in ascending order
        auto each = [&](auto&& f) {
            if (listed) {
                for (int e0 = 0; e0 < E; e0 += GE) {
                    const int e = e0 + el;
                    if (kok && e < E) f(list[e]);
                }
            } else {
                members(scan_mem, [&](int c, bool sel, int) { if (sel) f(c); });
            }
        };
        float sx = 0.f, sy = 0.f, qx = 0.f, qy = 0.f;
        float2 dm, m;
        if (listed && E <= 64) {                                 // one elite per lane: drawn once
            const bool act = kok && el < E;
            float2 u = mu;
            if (act) u = draw(list[el]);
            sx = act ? u.x - mu.x : 0.f; sy = act ? u.y - mu.y : 0.f;
            group_sum(sx, sy);
            dm = make_float2(sx / fE, sy / fE);
            m = make_float2(mu.x + dm.x, mu.y + dm.y);
            const float dx = act ? u.x - m.x : 0.f, dy = act ? u.y - m.y : 0.f;
            qx = dx * dx; qy = dy * dy;
            group_sum(qx, qy);
        } else {
            each([&](int c) { const float2 u = draw(c); sx += u.x - mu.x; sy += u.y - mu.y; });
            group_sum(sx, sy);
            dm = make_float2(sx / fE, sy / fE);
            m = make_float2(mu.x + dm.x, mu.y + dm.y);
            each([&](int c) {
                const float2 u = draw(c);
                const float dx = u.x - m.x, dy = u.y - m.y;
                qx += dx * dx; qy += dy * dy;
            });
            group_sum(qx, qy);
        }
        if (kok && el == 0) {
            const float keep = 1.0f - a.alpha;
            const float2 mean_new = make_float2(mu.x + a.alpha * dm.x, mu.y + a.alpha * dm.y);
            const float2 std_new = make_float2(fmaxf(a.sigma_min, keep * sd.x + a.alpha * sqrtf(qx / fE)),
                                               fmaxf(a.sigma_min, keep * sd.y + a.alpha * sqrtf(qy / fE)));
            if (k >= a.shift) { a.mean_out[t - (size_t)a.shift * bn] = mean_new; a.std_out[t - (size_t)a.shift * bn] = std_new; }
            if (a.shift && k == K - 1) { a.mean_out[t] = mean_new; a.std_out[t] = std_new; }
            if (k == 0 && a.act_out) a.act_out[row] = mean_new;
        }
    }
}

}  // namespace fg

#endif  // FG_PLANNER_KERNELS_HPP_
