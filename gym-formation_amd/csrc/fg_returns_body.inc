// fg_returns_body.inc - the body of returns_kernel, returns_sampled_kernel and returns_sampled_std_kernel (fg_returns_kernel.hpp,
// fg_planner_kernels.hpp): included inside each kernel, after `a` (const ReturnsArgs&) and the template parameters NC, G, T, with
// FG_RETURNS_SAMPLED 0 (the actions are read from a.act), 1 (they are drawn: `sa` is the kernel's ReturnsSampledArgs) or 2 (drawn
// with a sigma per element: `sa` is its ReturnsSampledStdArgs).  One `produce`, one recurrence; the kernels differ in where u
// comes from and in nothing else.  Included text and not a function: a
// call, even inlined, changes returns_kernel's instructions.
    static_assert(G <= 64 && T % 64 == 0 && 64 % G == 0 && G >= npad(NC), "a pair lives in one wave");
    constexpr int N = NC, NP = npad(NC), PW = T / G;
    constexpr int NPS = NP <= 16 ? NP : 0;              // small N: partners fetched up front (fg_pair_loops.hpp)
    extern __shared__ __attribute__((aligned(16))) real2 smem[];
    real* const smemf = reinterpret_cast<real*>(smem);
    const int tid = threadIdx.x;
    const int e = tid / G;
    const int i = tid % G;
    const uint32_t q = (uint32_t)blockIdx.x * PW + e;            // pair index: b C + c (the host checks B C < 2^31)
    const bool env_ok = q < (uint32_t)a.B * (uint32_t)a.C;
    const int b = env_ok ? (int)(q / (uint32_t)a.C) : 0;
    const int c = env_ok ? (int)(q - (uint32_t)b * (uint32_t)a.C) : 0;
    const bool valid = env_ok && (i < N);
    real* const QX = smemf + e * returns_block_floats(N);
    real* const QY = QX + NP; real* const PX = QY + NP; real* const PY = PX + NP;
    real* const SX = PY + NP; real* const SY = SX + NP;

    // (the constants of rollout_kernel, fg_rollout_kernels.hpp)
    const real one_minus_damp = 1.0f - a.p.damping;
    const real dt = a.p.dt;
    const real cutoff = a.p.dist_min + (FG_F64 ? 40.0f : 18.0f) * a.p.contact_margin;
    const real cutoff2 = cutoff * cutoff;
    const real thr2 = (real)((double)a.p.collide_thresh * (double)a.p.collide_thresh);
    const real invN = 1.0f / (real)N;

    real2 p = make_real2(0.f, 0.f), v = p, s = p, iv = p;
    int t_step = 0;
    const size_t sidx = (size_t)b * N + i;
    if (valid) {
        p = make_real2(a.px[sidx], a.py[sidx]);
        v = make_real2(a.vx[sidx], a.vy[sidx]);
        s = reinterpret_cast<const real2*>(a.shape)[sidx];
        QX[i] = p.x; QY[i] = p.y; SX[i] = s.x; SY[i] = s.y;
    } else if (env_ok && i < NP) {
        QX[i] = FAR_AWAY; QY[i] = FAR_AWAY; PX[i] = FAR_AWAY; PY[i] = FAR_AWAY; SX[i] = FAR_AWAY; SY[i] = FAR_AWAY;
    }
    if (env_ok) { iv = reinterpret_cast<const real2*>(a.ivel)[b]; t_step = a.step[b]; }
    // the steps that count: up to and including the one that sets the done flag (t_step + k + 1 >= world_length)
    const int nsteps = env_ok ? min(a.K, max(1, a.p.world_length - t_step)) : 0;

    // the action of step k + 1 is made during step k (two registers alternating over a loop unrolled by two, as the
    // producers of rollout_kernel do)
    real2 u_even = make_real2(0.f, 0.f), u_odd = u_even;
#if FG_RETURNS_SAMPLED
    // drawn from the plan's mean[k][b][i] - 8 N contiguous bytes per env and step, shared by the env's C candidates
    const size_t mean_stride = (size_t)a.B * N;                 // float2 units between consecutive steps
    const float2* mean_next = reinterpret_cast<const float2*>(sa.mean) + (size_t)(valid ? b : 0) * N + (valid ? i : 0);
#if FG_RETURNS_SAMPLED == 2
    // ... with the sigma of the same element, std[k][b][i], beside it
    const float2* std_next = reinterpret_cast<const float2*>(sa.sd) + (size_t)(valid ? b : 0) * N + (valid ? i : 0);
    if (valid) u_even = plan_draw_std(sa.d, *mean_next, *std_next, (uint32_t)b, (uint32_t)c, (uint32_t)i, 0u);
    std_next += a.K > 1 ? mean_stride : 0;
#else
    if (valid) u_even = plan_draw(sa.d, *mean_next, (uint32_t)b, (uint32_t)c, (uint32_t)i, 0u);
#endif
    mean_next += a.K > 1 ? mean_stride : 0;
#else
    // fetched from act[c][k][b][i]: a pair's step is 8 N contiguous bytes
    const size_t act_stride = (size_t)a.B * N;                  // real2 units between consecutive steps
    const real2* act_next = reinterpret_cast<const real2*>(a.act) + ((size_t)c * a.K * a.B + (valid ? b : 0)) * N + (valid ? i : 0);
    if (valid) u_even = *act_next;
    act_next += a.K > 1 ? act_stride : 0;
#endif

    real disc = (real)1, ret_shared = (real)0, ret_own = (real)0;

    // one step: World.step + reward of step k, then the recurrence.  The statements between the two marks are those of
    // rollout_kernel's `produce` (fg_rollout_kernels.hpp: contact force, action force, integration, reductions, reward pass,
    // `shared` / `own`), in its order: under -ffp-contract=on identical source statements contract identically, which is what
    // makes every step's reward the rollout kernels' bits.
    auto produce = [&](int k, const real2& u_cur, real2& u_nxt) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        real2 u_act = u_cur;
        // ---- from rollout_kernel::produce ----
        if (valid) {
#if FG_RETURNS_SAMPLED
            // one 8-byte load, ten Philox rounds, a log, a square root, a sine and a cosine: independent work beside the
            // pair loops below, where returns_kernel has its load in flight; nothing is drawn past the last step
            if (k + 1 < a.K) {
#if FG_RETURNS_SAMPLED == 2
                u_nxt = plan_draw_std(sa.d, *mean_next, *std_next, (uint32_t)b, (uint32_t)c, (uint32_t)i, (uint32_t)(k + 1));
                std_next += mean_stride;
#else
                u_nxt = plan_draw(sa.d, *mean_next, (uint32_t)b, (uint32_t)c, (uint32_t)i, (uint32_t)(k + 1));
#endif
                mean_next += mean_stride;
            }
#else
            // always issued (clamped to the last step): with a known number of younger loads the
            // wait for u_cur can leave this prefetch in flight
            u_nxt = *act_next;
            act_next += (k + 2 < a.K) ? act_stride : 0;
#endif
            real2 f = contact_force_packed<NPS>(QX, QY, NP, i, p, a.p.contact_force, a.p.contact_margin,
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
        real sums[4] = {valid ? p.x : 0.f, valid ? p.y : 0.f, valid ? v.x : 0.f, valid ? v.y : 0.f};
        env_reduce<G, G, 4, R_SUM, R_SUM, R_SUM, R_SUM>(sums, nullptr);
        const real mx = sums[0] * invN, my = sums[1] * invN;
        const real mvx = sums[2] * invN, mvy = sums[3] * invN;
        real rowmin = INFINITY, colmin = INFINITY;
        int cnt = 0, arg_lm = 0, arg_ag = 0;
        if (valid)
            reward_pass_packed<false, NPS>(PX, PY, SX, SY, NP, p, p.x - mx, p.y - my, s.x + mx, s.y + my, thr2,
                                           rowmin, colmin, cnt, arg_lm, arg_ag);
        real red[3] = {valid ? rowmin : -INFINITY, valid ? colmin : -INFINITY, (real)cnt};
        env_reduce<G, G, 3, R_MAX, R_MAX, R_SUM, R_SUM>(red, nullptr);
        const real H = rsqrt_(rmax(red[0], red[1]));
        const real ex = iv.x - mvx, ey = iv.y - mvy;
        const real velterm = rsqrt_(ex * ex + ey * ey);
        const real shared = (real)(-(double)N * ((double)H + (double)velterm) - (double)red[2]);
        const real own = (-H - velterm) - (real)cnt;
        // ---- end of rollout_kernel::produce's statements ----
        // R_k = R_{k-1} + d_k r_k, d_{k+1} = d_k gamma: every product and every sum rounded on its own (never an fma)
        if (k < nsteps) {
            ret_shared = add_rn_(ret_shared, mul_rn_(disc, shared));
            ret_own = add_rn_(ret_own, mul_rn_(disc, own));
        }
        disc = mul_rn_(disc, a.gamma);
        if (valid) { QX[i] = p.x; QY[i] = p.y; }       // next step's partners
    };

    for (int k = 0; k < a.K; k += 2) {
        if (__all(k >= nsteps) != 0) break;              // nothing of this wave counts any more (every loop stays bounded by K)
        produce(k, u_even, u_odd);
        if (k + 1 < a.K) produce(k + 1, u_odd, u_even);
    }
    if (valid) {
        const size_t o = ((size_t)c * a.B + b) * N + i;
        a.ret[o] = ret_shared;
        if (a.indiv_ret) a.indiv_ret[o] = ret_own;
    }
    if (a.steps && env_ok && c == 0 && i == 0) a.steps[b] = nsteps;
