// fg_scn_lane_actor_body.inc - the one body of scn_lane_actor and scn_lane_actor_gauss (fg_scn_lane_actor_kernel.hpp).
// Included inside each kernel, whose scope provides the kernel arguments `a` (ScnArgs: a.do_phys = 1, a.act and a.near_ag
// unused), `w` (ActorW), `act_out`, the template parameters KIND, N, L, M, NBR, H, `constexpr bool SAMPLE` and `log_std` /
// `logp` (SAMPLE = false: nullptr).  Not a header: no guard.  (A textual include for the reason written at the top of
// fg_actor_rollout_body.inc.)  This body holds the producer's step, the block stream and layer 1 on the composed block (one
// padded K range); the LDS preload and everything after layer 1 are formation_hd_env's text: fg_actor_mlp_preload.inc and
// fg_actor_mlp.inc.  Nothing per-agent is declared here.
    static_assert(!FG_F64, "the actor rollout is an fp32 kernel");
    constexpr bool LNORM = false;                       // no LayerNorm actor in the landmark scenarios' launch
    constexpr ActorNormW nw{};
    constexpr bool GRU = false;                         // nor a recurrent one
    constexpr ActorGruW gw{};
    float* const gsm = nullptr;
    float* const hst = nullptr;
    constexpr bool OU = false;                          // nor one with OU noise
    constexpr ActorOuW ow{};
    float* const oust = nullptr;
    constexpr bool CAT = false;                         // nor a categorical one
    constexpr ActorCatW cw{};
    constexpr bool GUM = false;                         // nor one with Gumbel noise
    constexpr ActorGumW gum{};
    constexpr bool DB = false;                          // one hand-over block, two barriers per step
    constexpr int PW = 1, ENVS = FG_SCN_ACTOR_ENVS, NWW = FG_SCN_ACTOR_THREADS / 64;   // every wave streams
    constexpr int NE = N + M;
    constexpr int G = scn_group_lanes(NE);
    constexpr int D = scn_obs_dim(KIND, N, L, M, NBR);  // actor input width
    constexpr int U = N * D / 2;                        // float2 units per env
    constexpr int SU = scn_lane_pitch(U);
    constexpr bool BASIC = KIND == FG_SCN_BASIC;
    constexpr int BLOCK_UNITS = scn_lane_block_bytes(KIND, N, L, M, NBR, 1) / 8;
    constexpr int HS = actor_hstride(H), CB = H / 16, RT = FG_ACTOR_ROWS / 16;
    constexpr int WS = 4 * H;                           // floats of b1 | b2 | W3 in LDS
    constexpr int WB = 4;                               // ... and of the b3 | log_std slot behind them
    constexpr int TILES = (ENVS * N + FG_ACTOR_ROWS - 1) / FG_ACTOR_ROWS;
    static_assert(NE <= 8 && L <= 8, "one env per lane: a handful of entities");
    static_assert(H % 16 == 0 && D % 2 == 0 && RT == 2, "bad actor geometry");
    extern __shared__ __attribute__((aligned(16))) float2 smem_all[];
    float2* const smem = smem_all;
    float* const act_lds = reinterpret_cast<float*>(smem_all + BLOCK_UNITS);            // [64 N][2]
    float* const wsm = act_lds + 2 * ENVS * N;                                           // b1 | b2 | W3 | b3 | log_std
    float* const hbuf = wsm + WS + WB;

    const int tid = threadIdx.x, lane = tid & 63;
    // consecutive workgroup ids take consecutive 64-env spans within an XCD's eighth of the batch (scn_lane_kernel's map)
    const int per_xcd = (int)(gridDim.x >> 3);
    const int wg = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    const int b0 = wg * ENVS;
    if (b0 >= a.B) return;                              // uniform over the workgroup, before any barrier
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int slot = lane;                              // the lane's env inside the workgroup (producer wave)
    const int b = b0 + slot;
    const bool live = b < a.B;
    const int bl = live ? b : a.B - 1;                  // loads of a lane beyond the batch stay in range; it stores nothing
    const int El = min(ENVS, a.B - b0);
    const int KS = a.K;

#include "fg_actor_mlp_preload.inc"

    // the producer lane's env (wave 0; the other waves never touch these)
    float2 p[NE], v[NE], lm[L];
    int t_step = 0;
    bool fresh_lm = false;                              // landmarks re-drawn by an in-launch reset: written back at the end
    const float k_margin = a.p.contact_margin;
    const float half_agent = 0.5f * a.p.dist_min, half_obst = 0.5f * (2.0f * a.sc.obstacle_size);
    const float thr = a.p.collide_thresh, thr2 = (float)((double)thr * (double)thr);
    const float ot = 0.5f * a.p.dist_min + a.sc.obstacle_size, ot2 = (float)((double)ot * (double)ot);
    const uint64_t rbase = rng_base(a.p);

    // ---- the actor on the block: act_lds[q] = actor(row q), q = env-major row (env q / N, agent q % N), and the same values
    // to act_out[kstep] (SAMPLE: plus exp(log_std) eps, eps drawn at counter offset `off`, log-density to logp[kstep]) ----
    const int rows = El * N;                            // rows that are agents of this workgroup
    auto actor = [&](uint64_t off, int kstep) {
        float* const hb = hbuf + wave * FG_ACTOR_ROWS * HS;
        const float* const blk = reinterpret_cast<const float*>(smem_all);
        const int col = lane & 15, kq = lane >> 4;      // MFMA operand lane map: row / column lane & 15, k = lane >> 4
        const size_t out0 = ((size_t)kstep * a.B + b0) * N;
        for (int t = wave; t < TILES; t += NWW) {
            const int q0 = t * FG_ACTOR_ROWS;
            int x0[RT];                                 // this lane's A-operand row in each 16-row tile: its first float
            bool row_ok[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int q = q0 + rt * 16 + col;
                row_ok[rt] = q < rows;
                const int qq = row_ok[rt] ? q : 0;
                const int ee = qq / N;
                x0[rt] = ee * (2 * SU) + (qq - ee * N) * D;
            }
            f32x4 acc[RT][CB];
            // ---- layer 1: K = D padded up to a multiple of 4 with zero operands ----
            actor_bias_init(acc, wsm, col);
            // (opaque per pass: the weight fragments do not depend on the tile, and hoisted out of the tile loop they would all
            // be held in registers)
            const float* w1row = w.w1 + (size_t)col * D;
            asm volatile("" : "+v"(w1row));
#pragma unroll 2
            for (int kc = 0; kc < (D + 3) / 4; ++kc) {
                const int k = kc * 4 + kq;
                const bool k_ok = k < D;
                const int kk = k_ok ? k : 0;            // padded k: an in-range address, a zero operand
                float xa[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const float x = blk[x0[rt] + kk];
                    xa[rt] = (row_ok[rt] && k_ok) ? x : 0.f;
                }
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) {
                    const float wv = w1row[cb * 16 * D + kk];
                    const float wb = k_ok ? wv : 0.f;
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
                        acc[rt][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[rt], wb, acc[rt][cb], 0, 0, 0);
                }
            }
#include "fg_actor_mlp.inc"
            if constexpr (SAMPLE) {
                if (logp && q < rows && o == 0) logp[out0 + q] = gauss_logp(n, ls0, ls1);
            }
            if (q < rows) {
                act_lds[2 * q + o] = y;
                act_out[2 * out0 + 2 * q + o] = y;         // the wave's 32 rows: 256 contiguous bytes
            }
            WaveSync()();                              // the tile is free for the next pass
        }
    };

    if (wave == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const size_t s = (size_t)bl * N + i;
            p[i] = make_float2(a.px[s], a.py[s]);
            v[i] = make_float2(a.vx[s], a.vy[s]);
        }
#pragma unroll
        for (int k = 0; k < M; ++k) {
            p[N + k] = reinterpret_cast<const float2*>(a.opos)[(size_t)bl * M + k];
            v[N + k] = reinterpret_cast<const float2*>(a.ovel)[(size_t)bl * M + k];
        }
#pragma unroll
        for (int l = 0; l < L; ++l) lm[l] = reinterpret_cast<const float2*>(a.lm)[(size_t)bl * L + l];
        t_step = a.step ? a.step[bl] : 0;
        // the observation of the current state (no physics): what step 0 acts on
        const bool want_obs = true;
#include "fg_scn_lane_compose.inc"
    }
    __syncthreads();
    actor(rbase, 0);
    __syncthreads();

    for (int ks = 0; ks < KS; ++ks) {
        if (wave == 0) {
            const uint64_t off = rbase + (uint64_t)ks;
            const size_t kb = (size_t)ks * a.B;
            float2 u_now[N];
#pragma unroll
            for (int i = 0; i < N; ++i)
                u_now[i] = live ? reinterpret_cast<const float2*>(act_lds)[slot * N + i] : make_float2(0.f, 0.f);
#include "fg_scn_lane_step.inc"
            float* const s_rew = reinterpret_cast<float*>(smem + ENVS * SU);
            float* const s_ind = s_rew + ENVS * N;
            uint32_t* const s_done = reinterpret_cast<uint32_t*>(s_ind + ENVS * N);
#pragma unroll
            for (int i = 0; i < N; ++i) {
                s_rew[slot * N + i] = shared; s_ind[slot * N + i] = indiv[i]; s_done[slot * N + i] = done_flag;
            }
            const bool want_obs = true;                 // composed every step: the block is the actor's input
#include "fg_scn_lane_compose.inc"
        }
        __syncthreads();                                // B: published
        {   // ---- the step's block -> global memory, all four waves ----
            const int wv = wave;
            const int B = a.B, obs_every = a.obs_every;
            float* const __restrict__ obs = a.obs; float* const __restrict__ rew = a.rew;
            float* const __restrict__ indiv = a.indiv; uint8_t* const __restrict__ done = a.done;
            {
                const int w = wv;                       // (the writer wave's index in fg_scn_lane_write.inc)
#include "fg_scn_lane_write.inc"
            }
        }
        if (ks + 1 < KS) actor(rbase + (uint64_t)(ks + 1), ks + 1);    // step ks + 1 draws at its own offset
        __syncthreads();                                // A: the block and the actions of step ks have been read
    }
    if (wave == 0 && live) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const size_t s = (size_t)b * N + i;
            a.px[s] = p[i].x; a.py[s] = p[i].y; a.vx[s] = v[i].x; a.vy[s] = v[i].y;
        }
#pragma unroll
        for (int k = 0; k < M; ++k) {
            reinterpret_cast<float2*>(a.opos)[(size_t)b * M + k] = p[N + k];
            reinterpret_cast<float2*>(a.ovel)[(size_t)b * M + k] = v[N + k];
        }
        if (fresh_lm) {
#pragma unroll
            for (int l = 0; l < L; ++l) reinterpret_cast<float2*>(a.lm)[(size_t)b * L + l] = lm[l];
        }
        if (a.step) a.step[b] = t_step;
    }
