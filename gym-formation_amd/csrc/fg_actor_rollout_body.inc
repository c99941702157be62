// fg_actor_rollout_body.inc - the one body of every formation_hd_env actor kernel: each member of each family block of
// fg_actor_rollout_kernel.hpp.  Included inside each kernel (fg_actor_family.inc), whose scope provides NC and H, the member and
// the family's flags (FG_ACTOR_IS: MEMBER and FLAGS, and from them the nine `constexpr bool`s the branches below test), the
// kernel arguments `a` (Args) and `w tab nw gw bw btab ow cw gum`, `log_std` / `logp` and `obs_fmt` - each a kernel parameter where
// the family or the member takes it, and an empty constant, nullptr or 0 where it does not.  The LDS blocks are
// actor_lds_layout's, the function the host sizes the launch with.
//   PER_AGENT  `tab` (ActorTab) instead of `w` (ActorW), of which only `w.out_tanh` is read; its layers 1 to 3 are here.
//   LNORM      `nw` (ActorNormW): the hidden LayerNorms are fg_actor_mlp.inc's, the input LayerNorm (nw.in_norm, wave-uniform)
//              is here - row statistics from the tables, then layer 1 over the whole k range on the normalised operand.
//   GRU        `gw` (ActorGruW), an LNORM body whose pass runs fg_actor_gru.inc between the second hidden norm and layer 3; here
//              are the hidden state's block - loaded from gw.state before the first pass, its done envs' rows zeroed by the
//              physics phase, stored back after the last step (the record gw.states is fg_actor_gru.inc's) - and the preload
//              of the layer's biases and norm.
//   INBN       `bw` (ActorBnW) or `btab` (ActorBnTab, PER_AGENT): layer 1's A operand through bn_apply, over the whole k range;
//              the shared actor's tables are filled here once per workgroup, the per-agent ones read through L1 per element.
//   SAMPLE     `log_std` / `logp`: the Gaussian step of layer 3's lanes (fg_actor_mlp.inc; the per-agent branch here) and the
//              log-probs' block, which the physics phase stores.
//   OU         `ow` (ActorOuW): the noise state's block - loaded from ow.state before the first pass, stepped by layer 3's lanes,
//              its done envs' rows set to mu by the physics phase, stored back after the last step.
//   CAT        `cw` (ActorCatW): the five-output head of fg_actor_mlp.inc leaves the decoded action in the actions' block and
//              the row's index and log-prob in two blocks [E N] behind it; the physics phase stores the three.
//   GUM        `gum` (ActorGumW): the five-output head under Gumbel noise - fg_actor_mlp.inc's for the shared families, the
//              per-agent branch here - leaves the decoded action in the actions' block and the row's index in the block [E N]
//              behind it; the physics phase stores the two.  There is no log-prob block.
//   OBS16      `obs_fmt`: the stream phase stores fp16 / bf16 units through write_obs16 (fg_obs_writers.hpp) instead of
//              write_obs_rows, the format a run-time, wave-uniform fact of the launch; its tile is the wave's activation tile.
// Not a header: no guard.
// This body holds the physics, the observation stream and layer 1 on the observation tables (two K ranges); what follows
// layer 1 for the shared actor - layers 2 and 3, the tanh, the Gaussian step - is fg_actor_mlp.inc, shared with the landmark
// scenarios' body, as is the LDS preload (fg_actor_mlp_preload.inc).  The per-agent branches stay here.
//
// Why a textual include and not a force-inlined __device__ function: behind a function boundary the kernel arguments reach
// the body through a by-value copy, and even inlined early the copy changes how the arguments are loaded and the order in
// which the address arithmetic is canonicalised - the deterministic kernel's ISA changed (kernarg loads split and sunk into
// branches, different registers).  Expanded in place, `if constexpr (SAMPLE)` leaves actor_rollout_kernel exactly the code
// it was before the sampling kernel existed.
    static_assert(!FG_F64, "the actor rollout is an fp32 kernel");
    constexpr int N = NC, NP = npad(NC), G = actor_lanes(NC), E = actor_envs(NC);
    constexpr int NPS = NP <= 16 ? NP : 0;
    constexpr int D = 6 * N;                           // actor input width
    constexpr int HS = actor_hstride(H), CB = H / 16, RT = FG_ACTOR_ROWS / 16, NW = FG_ACTOR_THREADS / 64;
    // PER_AGENT: the actor rows are agent-major - agent r owns rows r EP .. r EP + EP - 1, the workgroup's envs padded to
    // EP >= 16 - so that every 16-row MFMA tile holds one agent and takes that agent's weights as its B operand
    constexpr int EP = E >= 16 ? E : 16;
    constexpr int TILES = ((PER_AGENT ? EP * N : E * N) + FG_ACTOR_ROWS - 1) / FG_ACTOR_ROWS;
    constexpr int WS = actor_w_floats(H, PER_AGENT, CAT || GUM);   // floats of b1 | b2 | W3 in LDS (PER_AGENT: read through L1)
    constexpr int WB = actor_b3_floats(CAT || GUM);     // ... and of the b3 | log_std slot behind them
    static_assert(!CAT || (!SAMPLE && !OU && !PER_AGENT && !INBN), "the categorical actor: a shared body, no Gaussian or OU noise");
    static_assert(!GUM || (!SAMPLE && !OU && !CAT && !OBS16 && !LNORM && !GRU), "the Gumbel actor: a body without LayerNorms, no other noise");
    static_assert(!PER_AGENT || (RT == 2 && (EP & (EP - 1)) == 0), "per-agent rows: two tiles per pass, EP a power of two");
    constexpr int DP = actor_in_pad(N);                 // the input width rounded up to 4: the input norms' tables
    static_assert(!LNORM || !PER_AGENT, "the LayerNorm actor is a shared actor");
    static_assert(!GRU || LNORM, "the recurrent actor's base is the LayerNorm body");
    static_assert(!(INBN && LNORM), "the input BatchNorm is in front of the plain body only");
    static_assert(!INBN || H <= 64, "the BatchNorm actor's kernels: H 32 or 64");
    static_assert(!OU || (!SAMPLE && !LNORM && !GRU), "the OU-noise actor: a deterministic body without LayerNorms");
    static_assert(G <= 64 && NP <= G && E % NW == 0 && H % 16 == 0, "bad actor rollout geometry");
    extern __shared__ __attribute__((aligned(16))) float2 smem[];
    float* const smemf = reinterpret_cast<float*>(smem);
    // The blocks by actor_lds_layout's offsets.  Each pointer is chained from logp_lds, wsm or hbuf, not taken from `smemf`
    // directly: the compiler allocates registers differently in some kernels when it is.
    constexpr ActorLds L = actor_lds_layout(N, H, FLAGS, MEMBER);
    float2* const act_lds = reinterpret_cast<float2*>(smemf + L.act);
    float* const logp_lds = smemf + L.logp;             // SAMPLE and CAT only
    int* const idx_lds = reinterpret_cast<int*>(logp_lds + (L.idx - L.logp));   // CAT and GUM only
    float* const wsm = logp_lds + (L.wsm - L.logp);     // b1 | b2 | W3 | b3 | log_std
    float* const ln0 = wsm + (L.ln - L.wsm) + 4 * H;    // LNORM: behind the hidden norms' four [H], gamma0 [DP] | beta0 [DP], zeros at k >= D
    float* const bn0 = wsm + (L.bn - L.wsm);            // INBN, shared: mean | istd | gamma | beta [DP] each, zeros at k >= D
    float* const gsm = wsm + (L.gru - L.wsm);           // GRU: b_ir + b_hr | b_iz + b_hz | b_in | b_hn | gamma3 | beta3
    float* const hbuf = wsm + (L.tiles - L.wsm);
    float* const hst = hbuf + (L.state - L.tiles);      // GRU: the hidden state, row q of the workgroup at hst + q HS
    float* const oust = hbuf + (L.state - L.tiles);     // OU: the noise state, component o of env-major slot q at oust + 2 q + o
    static_assert(!GRU || L.state % 4 == 0,
                  "the hidden state's block is 16-byte aligned (fg_actor_gru.inc stores its rows with 16-byte reads)");

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

    if constexpr (!PER_AGENT) {
#include "fg_actor_mlp_preload.inc"
    } else if constexpr (SAMPLE) {
        if (tid < 2) wsm[WS + 2 + tid] = log_std[tid];
    }
    if constexpr (LNORM) {
        if (nw.in_norm) {
            for (int q = tid; q < DP; q += FG_ACTOR_THREADS) {
                ln0[q] = q < D ? (nw.g0 ? nw.g0[q] : 1.f) : 0.f;
                ln0[DP + q] = (q < D && nw.be0) ? nw.be0[q] : 0.f;
            }
        }
    }
    if constexpr (INBN && !PER_AGENT) {
        for (int q = tid; q < DP; q += FG_ACTOR_THREADS) {
            const bool in = q < D;
            bn0[q] = in ? bw.mean[q] : 0.f;
            bn0[DP + q] = in ? bn_istd(bw.var[q], bw.eps) : 0.f;
            bn0[2 * DP + q] = in ? (bw.gamma ? bw.gamma[q] : 1.f) : 0.f;
            bn0[3 * DP + q] = (in && bw.beta) ? bw.beta[q] : 0.f;
        }
    }

    if constexpr (GRU) {
        for (int q = tid; q < H; q += FG_ACTOR_THREADS) {
            gsm[q] = gw.b_ih[q] + gw.b_hh[q];
            gsm[H + q] = gw.b_ih[H + q] + gw.b_hh[H + q];
            gsm[2 * H + q] = gw.b_ih[2 * H + q];
            gsm[3 * H + q] = gw.b_hh[2 * H + q];
            gsm[4 * H + q] = gw.g3 ? gw.g3[q] : 1.f;
            gsm[5 * H + q] = gw.be3 ? gw.be3[q] : 0.f;
        }
        // the state of this workgroup's rows (env-major, contiguous in gw.state); rows past them start at zero
        const float* const hsrc = gw.state + (size_t)b0 * N * H;
        const int live = El * N * H;
        for (int idx = tid; idx < actor_state_rows(N) * H; idx += FG_ACTOR_THREADS)
            hst[(idx / H) * HS + idx % H] = idx < live ? hsrc[idx] : 0.f;
    }

    if constexpr (OU) {                                // the state of this workgroup's rows (env-major, contiguous in ow.state)
        const float* const xsrc = ow.state + (size_t)b0 * N * 2;
        for (int idx = tid; idx < E * N * 2; idx += FG_ACTOR_THREADS) oust[idx] = idx < El * N * 2 ? xsrc[idx] : ow.mu;
    }

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
    // (SAMPLE: plus exp(log_std) eps, eps drawn at counter offset `off`, and logp_lds[e N + i] = its log-density)
    const int M = El * N;                              // rows that are agents of this workgroup
    auto actor = [&](uint64_t off) {
        float* const hb = hbuf + wave * FG_ACTOR_ROWS * HS;
        const int col = lane & 15, kq = lane >> 4;     // MFMA operand lane map: row / column lane & 15, k = lane >> 4
        for (int t = wave; t < TILES; t += NW) {
            const int q0 = t * FG_ACTOR_ROWS;
            // this lane's A-operand row in each 16-row tile: env, agent, its position (unit r of its own table)
            const float2* AT[RT];
            int r_of[RT];
            float2 pr[RT];
            bool row_ok[RT];
            int ra[RT];                                // PER_AGENT: the agent of each tile (wave-uniform)
            // (the table's pointers reach the kernel as generic pointers: cast to the global address space, so that the loads
            // are global_load with a scalar base instead of flat loads with a 64-bit address per lane)
            using gfloat = const __attribute__((address_space(1))) float;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int q = q0 + rt * 16 + col;
                if constexpr (PER_AGENT) {
                    ra[rt] = min((q0 + rt * 16) / EP, N - 1);
                    const int ee = q % EP;
                    row_ok[rt] = ee < El && q / EP < N;
                    r_of[rt] = ra[rt];
                    AT[rt] = reinterpret_cast<const float2*>(smemf + (row_ok[rt] ? ee : 0) * env_block_floats(N));
                } else {
                    row_ok[rt] = q < M;
                    const int qq = row_ok[rt] ? q : 0;
                    const int ee = qq / N;
                    r_of[rt] = qq - ee * N;
                    AT[rt] = reinterpret_cast<const float2*>(smemf + ee * env_block_floats(N));
                }
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
            // LNORM with an input norm: each row's mean and rstd over all D features (x_in is zero at k >= D), a quarter of
            // the row per k lane, then the two steps across the four lanes that share the row
            constexpr int KA = (2 * N + 3) / 4, KB0 = (4 * N - 2) / 4, KB1 = (D + 3) / 4;
            const bool in_norm = LNORM && nw.in_norm != 0;
            float xmean[RT] = {}, xrstd[RT] = {};
            if constexpr (LNORM) {
                if (in_norm) {
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        float sum = 0.f;
                        for (int ks = 0; ks < KB1; ++ks) sum += x_in(rt, ks * 4 + kq);
                        sum = bfly<32, R_SUM>(bfly<16, R_SUM>(sum));
                        const float mean = sum * (1.0f / (float)D);
                        float ssq = 0.f;
                        for (int ks = 0; ks < KB1; ++ks) {
                            const int k = ks * 4 + kq;
                            const float d = k < D ? x_in(rt, k) - mean : 0.f;
                            ssq = __builtin_fmaf(d, d, ssq);
                        }
                        ssq = bfly<32, R_SUM>(bfly<16, R_SUM>(ssq));
                        xmean[rt] = mean;
                        xrstd[rt] = 1.0f / sqrtf(ssq * (1.0f / (float)D) + nw.eps0);
                    }
                }
            }
            f32x4 acc[RT][CB];
            // ---- layer 1: relative positions and velocity (k < 2N), then ideal shape and velocity (k >= 4N - 2) ----
            // PER_AGENT: each tile its own agent's bias and weight rows (the same two agents for the whole pass)
            auto bias_init = [&](int layer) {
#pragma unroll
                for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        gfloat* const bv = (gfloat*)(layer == 1 ? tab.b1[ra[rt]] : tab.b2[ra[rt]]);
                        const float bias = bv ? bv[cb * 16 + col] : 0.f;
                        acc[rt][cb] = (f32x4){bias, bias, bias, bias};
                    }
            };
            if constexpr (PER_AGENT) {
                bias_init(1);
            } else {
                actor_bias_init(acc, wsm, col);
            }
            // (opaque per pass: the weight fragments do not depend on the tile, and hoisted out of the tile loop they would all
            // be held in registers)
            const float* w1row = w.w1 + (size_t)col * D;
            // PER_AGENT: each tile's agent's weights, scalar bases; the lane's row offset is made opaque per k chunk, so that
            // the fragments of later chunks are not all loaded ahead into registers
            gfloat* w1pa[RT];
            if constexpr (PER_AGENT) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) w1pa[rt] = (gfloat*)tab.w1[ra[rt]];
            } else {
            asm volatile("" : "+v"(w1row));
            }
            auto l1_chunk = [&](int ks) {
                const int k = ks * 4 + kq;
                int ro = 0;
                if constexpr (PER_AGENT) {
                    ro = col * D;
                    asm volatile("" : "+v"(ro));
                }
                float xa[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) xa[rt] = x_in(rt, k);
                if constexpr (LNORM) {
                    if (in_norm) {                     // k < DP: gamma0 = beta0 = 0 at k >= D
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
                            xa[rt] = __builtin_fmaf((xa[rt] - xmean[rt]) * xrstd[rt], ln0[k], ln0[DP + k]);
                    }
                }
                if constexpr (INBN) {                  // k < DP: every operand 0 at k >= D, so x' = 0 there
                    if constexpr (PER_AGENT) {         // the tile's agent's statistics through L1 (scalar bases)
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) {
                            gfloat* const bm = (gfloat*)btab.mean[ra[rt]];
                            gfloat* const bv = (gfloat*)btab.var[ra[rt]];
                            gfloat* const bg = (gfloat*)btab.gamma[ra[rt]];
                            gfloat* const bb = (gfloat*)btab.beta[ra[rt]];
                            const bool in = k < D;
                            const float mean = in ? bm[k] : 0.f;
                            const float istd = in ? bn_istd(bv[k], btab.eps[ra[rt]]) : 0.f;
                            const float gamma = in ? (bg ? bg[k] : 1.f) : 0.f;
                            const float beta = (in && bb) ? bb[k] : 0.f;
                            xa[rt] = bn_apply(xa[rt], mean, istd, gamma, beta);
                        }
                    } else {
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
                            xa[rt] = bn_apply(xa[rt], bn0[k], bn0[DP + k], bn0[2 * DP + k], bn0[3 * DP + k]);
                    }
                }
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) {
                    if constexpr (PER_AGENT) {
                        float wb[RT];
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) wb[rt] = k < D ? w1pa[rt][ro + cb * 16 * D + k] : 0.f;
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
                            acc[rt][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[rt], wb[rt], acc[rt][cb], 0, 0, 0);
                    } else {
                    const float wb = k < D ? w1row[cb * 16 * D + k] : 0.f;
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
                        acc[rt][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[rt], wb, acc[rt][cb], 0, 0, 0);
                    }
                }
            };
            static_assert(KB0 >= KA, "the two input blocks overlap");
            // (an input norm: the communication block too - its normalised zeros are not zero)
#pragma unroll 2
            for (int ks = 0; ks < KA; ++ks) l1_chunk(ks);
            if constexpr (LNORM) {
                if (in_norm) {
#pragma unroll 2
                    for (int ks = KA; ks < KB0; ++ks) l1_chunk(ks);
                }
            }
            if constexpr (INBN) {                      // an input BatchNorm likewise: beta - mean istd gamma there
#pragma unroll 2
                for (int ks = KA; ks < KB0; ++ks) l1_chunk(ks);
            }
#pragma unroll 2
            for (int ks = KB0; ks < KB1; ++ks) l1_chunk(ks);
            if constexpr (PER_AGENT) {
                actor_store_tile(hb, HS, acc, col, kq);
                WaveSync()();
                // ---- layer 2 ----
                bias_init(2);
                gfloat* w2pa[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) w2pa[rt] = (gfloat*)tab.w2[ra[rt]];
#pragma unroll 2
                for (int ks = 0; ks < H / 4; ++ks) {
                    const int k = ks * 4 + kq;
                    int ro = col * H;
                    asm volatile("" : "+v"(ro));
                    float xa[RT];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) xa[rt] = hb[(rt * 16 + col) * HS + k];
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb) {
                        float wb[RT];
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) wb[rt] = w2pa[rt][ro + cb * 16 * H + k];
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
                            acc[rt][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[rt], wb[rt], acc[rt][cb], 0, 0, 0);
                    }
                }
                WaveSync()();                          // every read of the layer-1 tile before it is overwritten
                actor_store_tile(hb, HS, acc, col, kq);
                WaveSync()();
                // ---- layer 3 on the VALU: lane = (row, output), the row's tile's agent through L1 ----
                const int row = lane >> 1, o = lane & 1;
                const float* const hr = hb + row * HS;
                gfloat* const b3 = (gfloat*)(row < 16 ? tab.b3[ra[0]] : tab.b3[ra[1]]);
                if constexpr (GUM) {
                    // a head of five: both lanes of a row evaluate the five ascending chains from b3[j] (the shared kernel's
                    // bits), draw for (env ee, agent r) of the agent-major row and pick; lane o writes component o
                    gfloat* const w3 = (gfloat*)(row < 16 ? tab.w3[ra[0]] : tab.w3[ra[1]]);
                    float l[FG_CAT];
#pragma unroll
                    for (int j = 0; j < FG_CAT; ++j) l[j] = b3 ? b3[j] : 0.f;
#pragma unroll 4
                    for (int k = 0; k < H; ++k) {
                        const float hk = hr[k];
#pragma unroll
                        for (int j = 0; j < FG_CAT; ++j) l[j] = __builtin_fmaf(hk, w3[j * H + k], l[j]);
                    }
                    const int q = q0 + row;
                    const int ee = q % EP, r = q / EP, slot = ee * N + r;
                    const bool ok = ee < El && r < N;
                    float gd[FG_CAT] = {};
                    if (gum.explore) actor_gumbel(a.p.seed, (uint32_t)(b0 + ee + a.p.env_index_base), (uint32_t)r, off, gd);
                    const int pk = gumbel_pick(l, gd, gum.explore != 0);
                    const float2 ua = cat_decode(gum.mode, pk);
                    if (ok) {
                        reinterpret_cast<float*>(act_lds)[2 * slot + o] = o ? ua.y : ua.x;
                        if (o == 0) idx_lds[slot] = pk;
                    }
                } else {
                gfloat* const w3 = (gfloat*)(row < 16 ? tab.w3[ra[0]] : tab.w3[ra[1]]) + o * H;
                float y = b3 ? b3[o] : 0.f;
#pragma unroll 8
                for (int k = 0; k < H; ++k) y = __builtin_fmaf(hr[k], w3[k], y);
                if (w.out_tanh) y = tanhf(y);
                const int q = q0 + row;
                // the row's env and agent (agent-major rows), whether it is one of this workgroup's, its env-major slot
                const int ee = q % EP, r = q / EP, slot = ee * N + r;
                const bool ok = ee < El && r < N;
                if constexpr (SAMPLE) {                // actor_sample_kernel's draw of (env, agent)
                    const float2 n = actor_eps(a.p.seed, (uint32_t)(b0 + ee + a.p.env_index_base), (uint32_t)r, off);
                    const float ls0 = wsm[WS + 2], ls1 = wsm[WS + 3];
                    y += __expf(o ? ls1 : ls0) * (o ? n.y : n.x);
                    if (ok && o == 0) logp_lds[slot] = gauss_logp(n, ls0, ls1);
                }
                if constexpr (OU) {                    // ou_actor_kernel's step of (env, agent): the same draw, the state's slot
                    const float2 n = actor_eps(a.p.seed, (uint32_t)(b0 + ee + a.p.env_index_base), (uint32_t)r, off);
                    if (ok) {
                        const float x = ou_step(oust[2 * slot + o], o ? n.y : n.x, ow.theta, ow.mu, ow.sigma);
                        oust[2 * slot + o] = x;
                        y = ou_action(y, x, ow.scale, ow.clip);
                    }
                }
                if (ok) reinterpret_cast<float*>(act_lds)[2 * slot + o] = y;
                }
            } else {
#include "fg_actor_mlp.inc"
                if constexpr (SAMPLE) {
                    if (q < M && o == 0) logp_lds[q] = gauss_logp(n, ls0, ls1);
                }
                if constexpr (CAT) {
                    if (q < M && o == 0) { idx_lds[q] = pick.idx; logp_lds[q] = pick.logp; }
                }
                if constexpr (GUM) {
                    if (q < M && o == 0) idx_lds[q] = pick.idx;
                }
                if (q < M) reinterpret_cast<float*>(act_lds)[2 * q + o] = y;
            }
            WaveSync()();                              // the tile is free for the next pass
        }
    };

    publish();
    __syncthreads();
    actor(rbase);                                      // the action of step 0: the observation of the current state
    __syncthreads();

    for (int k = 0; k < a.K; ++k) {
        // ---- physics: World.step + reward + done + auto-reset of step k (rollout_kernel's producer step) ----
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (valid) {
            const float2 u_act = act_lds[e * N + i];
            reinterpret_cast<float2*>(a.act_out)[((size_t)k * a.B + b) * N + i] = u_act;
            if constexpr (SAMPLE) {
                if (logp) logp[((size_t)k * a.B + b) * N + i] = logp_lds[e * N + i];
            }
            if constexpr (CAT) {
                cw.idx[((size_t)k * a.B + b) * N + i] = idx_lds[e * N + i];
                if (cw.logp) cw.logp[((size_t)k * a.B + b) * N + i] = logp_lds[e * N + i];
            }
            if constexpr (GUM) {
                gum.idx[((size_t)k * a.B + b) * N + i] = idx_lds[e * N + i];
            }
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
        if constexpr (GRU) {                           // h = h * ~done: the episode's memory ends with it
            if (is_done && valid) {
                float* const hr = hst + (e * N + i) * HS;
#pragma unroll 8
                for (int c = 0; c < H; ++c) hr[c] = 0.f;
            }
        }
        if constexpr (OU) {                            // reset_noise(): the next episode starts from mu
            if (is_done && valid) { oust[2 * (e * N + i)] = ow.mu; oust[2 * (e * N + i) + 1] = ow.mu; }
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
            if constexpr (OBS16) {
                // the wave's 16-bit tile in its own activation tile: only this wave touches either, the stream phase precedes
                // its actor pass in program order and LDS operations of a wave complete in order - no barrier.  ONE tile per
                // wave: at 3 and 9 agents a wave has one tile per step anyway, at 27 its up to six are composed and streamed in
                // turn (a second tile fits at H = 64 only, and with it gru_cat_actor_obs16<27,64> keeps a scratch slot).
                constexpr int OW = obs16_tile_words<NC, NW, E>(), OT = 1;
                static_assert(OT * OW <= FG_ACTOR_ROWS * HS, "the 16-bit tile fits the wave's activation tile");
                static_assert(L.tiles % 4 == 0 && (FG_ACTOR_ROWS * HS) % 4 == 0, "the 16-bit tiles start on a 16-byte boundary");
                write_obs16<NC, NW, E, FG_WR_OBS_RT, OT, FG_ACTOR_ROWS * HS>(
                    reinterpret_cast<const float2*>(smemf), env_block_floats(N) / 2, wave, reinterpret_cast<uint32_t*>(hbuf),
                    reinterpret_cast<uint32_t*>(a.obs) + unit0, unit0, El, obs_fmt);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the tiles' reads before the pass's stores (other types)
            } else {
            write_obs_rows<NC, NW, E>(reinterpret_cast<const float2*>(smemf), env_block_floats(N) / 2, wave,
                                      reinterpret_cast<float2*>(a.obs) + unit0, (size_t)a.obs_pitch, El, 3);
            }
        }
        if (k + 1 < a.K) actor(rbase + k + 1);         // step k + 1 draws at its own offset
        __syncthreads();
    }
    if (valid) {
        a.px[sidx] = p.x; a.py[sidx] = p.y; a.vx[sidx] = v.x; a.vy[sidx] = v.y;
    }
    if (a.step && env_ok && i == 0) a.step[b] = t_step;
    if constexpr (GRU) {                               // (the loop's last barrier ordered the last pass and the last masking)
        float* const hdst = gw.state + (size_t)b0 * N * H;
        for (int idx = tid; idx < El * N * H; idx += FG_ACTOR_THREADS) hdst[idx] = hst[(idx / H) * HS + idx % H];
    }
    if constexpr (OU) {                                // (likewise: the last pass's steps and the last step's resets)
        float* const xdst = ow.state + (size_t)b0 * N * 2;
        for (int idx = tid; idx < El * N * 2; idx += FG_ACTOR_THREADS) xdst[idx] = oust[idx];
    }
