// fg_actor_rollout_kernel.hpp - Closed-loop K-step rollout driven by the caller's MLP actor (fg_rollout_hd_actor).
// Part of libformation_hip (gfx950); included by formation_hip.hip.
//
// The loop of a learned actor, `a = actor(o); o, r, d, info = env.step(a)`, K times in ONE launch, with the actor
//     Linear(6N, H) - ReLU - Linear(H, H) - ReLU - Linear(H, 2) [- Tanh]
// shared by every agent (parameter sharing) and read in place from the caller's fp32 parameter tensors (torch Linear
// layout [out][in]; NULL biases are zero).
//
// Geometry (one per (N, H), no fill rules): 256 threads, G = N rounded up to a power of two (>= 4) lanes per env, E = 256 / G
// envs per workgroup.  Each step, in three phases separated by workgroup barriers:
//   physics  every lane runs World.step + reward + auto-reset of its agent with the device functions of rollout_kernel
//            (fg_pair_loops.hpp, the butterflies of fg_common.hpp, the same Philox counters) in the same order, so replaying
//            the recorded actions through fg_rollout_hd gives the same bits; it publishes the env's observation tables
//   stream   the four waves store the step's observations from the tables (write_obs_rows, fg_obs_writers.hpp) and then
//   actor    evaluate the MLP for the next step: the rows of the product are the workgroup's E x N agents, taken 32 at a time
//            per wave (two 16-row tiles sharing every weight fragment); layers 1 and 2 on v_mfma_f32_16x16x4_f32 (exact fp32,
//            one rounding per product) with the weights as the B operand straight from global memory (every workgroup reads
//            the same few tens of KiB: L2 / L1 hits), the activations through a per-wave LDS tile; layer 3 (two outputs) on
//            the VALU, one lane per (row, output).  Layer 1 reads its input straight from the tables - the units the
//            observation writers store - and skips the communication block (zero for silent agents).
// No atomics: two launches from the same state and weights give the same bits.
#ifndef FG_ACTOR_ROLLOUT_KERNEL_HPP_
#define FG_ACTOR_ROLLOUT_KERNEL_HPP_

#include "fg_common.hpp"
#include "fg_pair_loops.hpp"
#include "fg_obs_writers.hpp"
#include "fg_policy_kernels.hpp"      // WaveSync

namespace fg {

// the caller's actor as the kernel reads it (FgActor without the hidden width, which is a template parameter)
struct ActorW {
    const float* w1; const float* b1;         // [H][6N], [H]
    const float* w2; const float* b2;         // [H][H],  [H]
    const float* w3; const float* b3;         // [2][H],  [2]
    int out_tanh;
};

constexpr int FG_ACTOR_THREADS = 256;
constexpr int FG_ACTOR_ROWS = 32;             // rows of one wave pass: two 16-row MFMA tiles
__host__ __device__ constexpr int actor_lanes(int n) { return n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : 32; }
__host__ __device__ constexpr int actor_envs(int n) { return FG_ACTOR_THREADS / actor_lanes(n); }
__host__ __device__ constexpr int actor_hstride(int h) { return h + 4; }   // row pitch of the activation tile: 16 rows x 4 k conflict-free
// LDS (floats): env blocks [E][env_block_floats] | actions [E N][2] | b1 [H] b2 [H] W3 [2][H] b3 [2] (+2) | activations [4][32][H + 4]
template <int NC, int H> constexpr int actor_lds_floats() {
    return actor_envs(NC) * env_block_floats(NC) + 2 * actor_envs(NC) * NC + 4 * H + 4 +
           (FG_ACTOR_THREADS / 64) * FG_ACTOR_ROWS * actor_hstride(H);
}
template <int NC, int H> constexpr int actor_lds_bytes() { return actor_lds_floats<NC, H>() * (int)sizeof(float); }

template <int NC, int H>
__global__ __launch_bounds__(FG_ACTOR_THREADS) void actor_rollout_kernel(const Args a, const ActorW w) {
    static_assert(!FG_F64, "the actor rollout is an fp32 kernel");
    constexpr int N = NC, NP = npad(NC), G = actor_lanes(NC), E = actor_envs(NC);
    constexpr int NPS = NP <= 16 ? NP : 0;
    constexpr int D = 6 * N;                           // actor input width
    constexpr int HS = actor_hstride(H), CB = H / 16, RT = FG_ACTOR_ROWS / 16, NW = FG_ACTOR_THREADS / 64;
    constexpr int TILES = (E * N + FG_ACTOR_ROWS - 1) / FG_ACTOR_ROWS;
    static_assert(G <= 64 && NP <= G && E % NW == 0 && H % 16 == 0, "bad actor rollout geometry");
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    float* const smemf = reinterpret_cast<float*>(smem);
    float2* const act_lds = reinterpret_cast<float2*>(smemf + E * env_block_floats(N));
    float* const wsm = smemf + E * env_block_floats(N) + 2 * E * N;       // b1 | b2 | W3 | b3
    float* const hbuf = wsm + 4 * H + 4;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int e = tid / G, i = tid % G;
    const int b0 = (int)blockIdx.x * E;
    const int b = b0 + e;
    const bool env_ok = b < a.B;
    const bool valid = env_ok && i < N;
    const int El = min(E, a.B - b0);
    float* const blk = smemf + e * env_block_floats(N);
    float2* const A = reinterpret_cast<float2*>(blk);                    // A[3N] | V[N] | NV[N]
    float* const QX = blk + 10 * N;
    float* const QY = QX + NP; float* const PX = QY + NP; float* const PY = PX + NP;
    float* const SX = PY + NP; float* const SY = SX + NP;

    for (int q = tid; q < H; q += FG_ACTOR_THREADS) {
        wsm[q] = w.b1 ? w.b1[q] : 0.f;
        wsm[H + q] = w.b2 ? w.b2[q] : 0.f;
        wsm[2 * H + q] = w.w3[q];
        wsm[3 * H + q] = w.w3[H + q];
    }
    if (tid < 2) wsm[4 * H + tid] = w.b3 ? w.b3[tid] : 0.f;

    const float one_minus_damp = 1.0f - a.p.damping;
    const float dt = a.p.dt;
    const float cutoff = a.p.dist_min + 18.0f * a.p.contact_margin;
    const float cutoff2 = cutoff * cutoff;
    const float thr2 = (float)((double)a.p.collide_thresh * (double)a.p.collide_thresh);
    const float invN = 1.0f / (float)N;
    const uint64_t rbase = rng_base(a.p);

    float2 p = make_float2(0.f, 0.f), v = p, s = p, iv = p;
    int t_step = 0;
    const size_t sidx = (size_t)b * N + i;
    if (valid) {
        p = make_float2(a.px[sidx], a.py[sidx]);
        v = make_float2(a.vx[sidx], a.vy[sidx]);
        s = reinterpret_cast<const float2*>(a.shape)[sidx];
        QX[i] = p.x; QY[i] = p.y; SX[i] = s.x; SY[i] = s.y;
        if (i < N - 1) A[N + i] = make_float2(0.f, 0.f);                  // the communication block of silent agents
    } else if (env_ok && i < NP) {
        QX[i] = FAR_AWAY; QY[i] = FAR_AWAY; PX[i] = FAR_AWAY; PY[i] = FAR_AWAY; SX[i] = FAR_AWAY; SY[i] = FAR_AWAY;
    }
    if (env_ok) { iv = reinterpret_cast<const float2*>(a.ivel)[b]; if (a.step) t_step = a.step[b]; }
    auto publish = [&]() {                             // the observation tables of the state in registers
        if (valid) {
            A[i] = p; A[3 * N + i] = v; A[4 * N + i] = make_float2(-v.x, -v.y);
            A[2 * N - 1 + i] = s;
            if (i == 0) A[3 * N - 1] = iv;
            QX[i] = p.x; QY[i] = p.y;
        }
    };

    // ---- the actor on the published tables: act_lds[e N + i] = actor(observation row i of env e) ----
    const int M = El * N;                              // rows that are agents of this workgroup
    auto actor = [&]() {
        float* const hb = hbuf + wave * FG_ACTOR_ROWS * HS;
        const int col = lane & 15, kq = lane >> 4;     // MFMA operand lane map: row / column lane & 15, k = lane >> 4
        for (int t = wave; t < TILES; t += NW) {
            const int q0 = t * FG_ACTOR_ROWS;
            // this lane's A-operand row in each 16-row tile: env, agent, its position (unit r of its own table)
            const float2* AT[RT];
            int r_of[RT];
            float2 pr[RT];
            bool row_ok[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int q = q0 + rt * 16 + col;
                row_ok[rt] = q < M;
                const int qq = row_ok[rt] ? q : 0;
                const int ee = qq / N;
                r_of[rt] = qq - ee * N;
                AT[rt] = reinterpret_cast<const float2*>(smemf + ee * env_block_floats(N));
                pr[rt] = AT[rt][r_of[rt]];
            }
            // observation unit u of row r (as write_obs_rows stores it): 0 velocity, 1 .. N-1 p_j - p_r (j skips r),
            // N .. 2N-2 communication (zeros), 2N-1 .. 3N-2 ideal shape, 3N-1 ideal velocity
            auto x_in = [&](int rt, int k) -> float {
                const int u = k >> 1;
                const int r = r_of[rt];
                const bool rel = u >= 1 && u < N;
                const int idx = u == 0 ? 3 * N + r : (rel ? ((u - 1 >= r) ? u : u - 1) : u);
                const float2 val = AT[rt][u < 3 * N ? idx : 0];
                const float2 sub = rel ? pr[rt] : make_float2(0.f, 0.f);
                const float x = (k & 1) ? val.y - sub.y : val.x - sub.x;
                return (row_ok[rt] && k < D) ? x : 0.f;
            };
            f32x4 acc[RT][CB];
            // ---- layer 1: relative positions and velocity (k < 2N), then ideal shape and velocity (k >= 4N - 2) ----
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                const float bias = wsm[cb * 16 + col];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc[rt][cb] = (f32x4){bias, bias, bias, bias};
            }
            // (opaque per pass: the weight fragments do not depend on the tile, and hoisted out of the tile loop they would all
            // be held in registers)
            const float* w1row = w.w1 + (size_t)col * D;
            asm volatile("" : "+v"(w1row));
            auto l1_chunk = [&](int ks) {
                const int k = ks * 4 + kq;
                float xa[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) xa[rt] = x_in(rt, k);
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) {
                    const float wb = k < D ? w1row[cb * 16 * D + k] : 0.f;
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
                        acc[rt][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[rt], wb, acc[rt][cb], 0, 0, 0);
                }
            };
            constexpr int KA = (2 * N + 3) / 4, KB0 = (4 * N - 2) / 4, KB1 = (D + 3) / 4;
            static_assert(KB0 >= KA, "the two input blocks overlap");
#pragma unroll 2
            for (int ks = 0; ks < KA; ++ks) l1_chunk(ks);
#pragma unroll 2
            for (int ks = KB0; ks < KB1; ++ks) l1_chunk(ks);
            // ReLU -> activation tile: accumulator register j of lane l is row 4 (l >> 4) + j, column l & 15
            auto store_tile = [&]() {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            hb[(rt * 16 + kq * 4 + j) * HS + cb * 16 + col] = fmaxf(acc[rt][cb][j], 0.f);
            };
            store_tile();
            WaveSync()();
            // ---- layer 2 ----
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) {
                const float bias = wsm[H + cb * 16 + col];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) acc[rt][cb] = (f32x4){bias, bias, bias, bias};
            }
            const float* w2row = w.w2 + (size_t)col * H;
            asm volatile("" : "+v"(w2row));
#pragma unroll 2
            for (int ks = 0; ks < H / 4; ++ks) {
                const int k = ks * 4 + kq;
                float xa[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) xa[rt] = hb[(rt * 16 + col) * HS + k];
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) {
                    const float wb = w2row[cb * 16 * H + k];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
                        acc[rt][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[rt], wb, acc[rt][cb], 0, 0, 0);
                }
            }
            WaveSync()();                              // every read of the layer-1 tile before it is overwritten
            store_tile();
            WaveSync()();
            // ---- layer 3 on the VALU: lane = (row, output) ----
            {
                const int row = lane >> 1, o = lane & 1;
                const float* const hr = hb + row * HS;
                const float* const w3 = wsm + 2 * H + o * H;
                float y = wsm[4 * H + o];
#pragma unroll 8
                for (int k = 0; k < H; ++k) y = __builtin_fmaf(hr[k], w3[k], y);
                if (w.out_tanh) y = tanhf(y);
                const int q = q0 + row;
                if (q < M) reinterpret_cast<float*>(act_lds)[2 * q + o] = y;
            }
            WaveSync()();                              // the tile is free for the next pass
        }
    };

    publish();
    __syncthreads();
    actor();                                           // the action of step 0: the observation of the current state
    __syncthreads();

    for (int k = 0; k < a.K; ++k) {
        // ---- physics: World.step + reward + done + auto-reset of step k (rollout_kernel's producer step) ----
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (valid) {
            const float2 u_act = act_lds[e * N + i];
            reinterpret_cast<float2*>(a.act_out)[((size_t)k * a.B + b) * N + i] = u_act;
            float2 f = contact_force_packed<NPS>(QX, QY, NP, i, p, a.p.contact_force, a.p.contact_margin,
                                                 a.p.dist_min, cutoff2);
            f.x += a.p.mass * (a.p.sensitivity * u_act.x);
            f.y += a.p.mass * (a.p.sensitivity * u_act.y);
            v.x = v.x * one_minus_damp + (f.x / a.p.mass) * dt;
            v.y = v.y * one_minus_damp + (f.y / a.p.mass) * dt;
            p.x += v.x * dt;
            p.y += v.y * dt;
            PX[i] = p.x; PY[i] = p.y;
        }
        t_step += 1;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float sums[4] = {valid ? p.x : 0.f, valid ? p.y : 0.f, valid ? v.x : 0.f, valid ? v.y : 0.f};
        env_reduce<G, G, 4, R_SUM, R_SUM, R_SUM, R_SUM>(sums, nullptr);
        const float mx = sums[0] * invN, my = sums[1] * invN;
        const float mvx = sums[2] * invN, mvy = sums[3] * invN;
        float rowmin = INFINITY, colmin = INFINITY;
        int cnt = 0, arg_lm = 0, arg_ag = 0;
        if (valid)
            reward_pass_packed<false, NPS>(PX, PY, SX, SY, NP, p, p.x - mx, p.y - my, s.x + mx, s.y + my, thr2,
                                           rowmin, colmin, cnt, arg_lm, arg_ag);
        float red[3] = {valid ? rowmin : -INFINITY, valid ? colmin : -INFINITY, (float)cnt};
        env_reduce<G, G, 3, R_MAX, R_MAX, R_SUM, R_SUM>(red, nullptr);
        const float Hd = rsqrt_(rmax(red[0], red[1]));
        const float ex = iv.x - mvx, ey = iv.y - mvy;
        const float velterm = rsqrt_(ex * ex + ey * ey);
        const bool is_done = t_step >= a.p.world_length;
        if (valid) {
            const size_t o = ((size_t)k * a.B + b) * N + i;
            a.rew[o] = (float)(-(double)N * ((double)Hd + (double)velterm) - (double)red[2]);
            if (a.indiv) a.indiv[o] = (-Hd - velterm) - (float)cnt;
            if (a.done) a.done[o] = is_done ? 1 : 0;
        }
        if (a.p.auto_reset) {
            const bool mine = is_done && env_ok;
            if (__any(mine) != 0) {
                uint32_t c[4] = {(uint32_t)(b + a.p.env_index_base), (uint32_t)i, (uint32_t)(rbase + k),
                                 (uint32_t)((rbase + k) >> 32)};
                philox4x32(c, (uint32_t)a.p.seed, (uint32_t)(a.p.seed >> 32));
                float raw[2] = {valid ? u_pm1(c[2]) : 0.f, valid ? u_pm1(c[3]) : 0.f};
                const float rx = raw[0], ry = raw[1];
                env_reduce<G, G, 2, R_SUM, R_SUM, R_SUM, R_SUM>(raw, nullptr);
                uint32_t c2[4] = {(uint32_t)(b + a.p.env_index_base), 0xFFFFFFFFu, (uint32_t)(rbase + k),
                                  (uint32_t)((rbase + k) >> 32)};
                philox4x32(c2, (uint32_t)a.p.seed, (uint32_t)(a.p.seed >> 32));
                if (mine) {
                    iv = make_float2(u_pm1(c2[0]), u_pm1(c2[1]));
                    t_step = 0;
                    if (valid) {
                        p = make_float2(u_pm1(c[0]), u_pm1(c[1]));
                        v = make_float2(0.f, 0.f);
                        s = make_float2(rfma(-raw[0], invN, rx), rfma(-raw[1], invN, ry));
                        SX[i] = s.x; SY[i] = s.y;
                        reinterpret_cast<float2*>(a.shape)[sidx] = s;
                        if (i == 0) reinterpret_cast<float2*>(a.ivel)[b] = iv;
                    }
                }
            }
        }
        publish();
        __syncthreads();
        // ---- the step's observations, then the actor for step k + 1 on the same tables ----
        int slot = k;
        bool want_obs = a.obs != nullptr;
        if (a.obs_every > 1) { want_obs = want_obs && ((k + 1) % a.obs_every == 0); slot = k / a.obs_every; }
        if (want_obs) {
            const size_t unit0 = ((size_t)slot * a.B + b0) * (size_t)a.obs_pitch;
            write_obs_rows<NC, NW, E>(reinterpret_cast<const float2*>(smemf), env_block_floats(N) / 2, wave,
                                      reinterpret_cast<float2*>(a.obs) + unit0, (size_t)a.obs_pitch, El, 3);
        }
        if (k + 1 < a.K) actor();
        __syncthreads();
    }
    if (valid) {
        a.px[sidx] = p.x; a.py[sidx] = p.y; a.vx[sidx] = v.x; a.vy[sidx] = v.y;
    }
    if (a.step && env_ok && i == 0) a.step[b] = t_step;
}

}  // namespace fg

#endif  // FG_ACTOR_ROLLOUT_KERNEL_HPP_
