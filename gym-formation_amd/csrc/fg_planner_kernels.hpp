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

}  // namespace fg

#endif  // FG_PLANNER_KERNELS_HPP_
