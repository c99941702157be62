// fg_scn_lane_step.inc - one step of a lane's environment in the one-env-per-lane kernels: World.step, formation / collision
// reward, done flag and in-launch auto-reset, exactly as scn_lane_kernel's producer does them (fg_scn_lane_kernel.hpp), shared
// with scn_lane_actor (fg_scn_lane_actor_kernel.hpp) so that replaying its recorded actions gives the same bits.  Included
// inside the step loop, whose scope provides: the kernel arguments `a` (ScnArgs), KIND, N, L, M, NE, G, BASIC (constants), the
// lane's state p, v, lm, t_step, fresh_lm, its env b / live, the step's action u_now[N], ks, kb, off and the launch constants
// k_margin, half_agent, half_obst, thr2, ot2.  Leaves form, cnt, total, is_done, shared, indiv[N], done_flag.
// Not a header: no guard.  A textual include for the reason written at the top of fg_actor_rollout_body.inc.
        if (a.do_phys) {
            // ---- World.step: every pair once, in lexicographic order - which is ascending j for each entity, the
            // order core.py:240-262 (and scn_kernel) accumulates in; the pair's two forces are exact negatives
            float fx[NE], fy[NE];
#pragma unroll
            for (int i = 0; i < NE; ++i) { fx[i] = 0.f; fy[i] = 0.f; }
#pragma unroll
            for (int i = 0; i < NE; ++i) {
#pragma unroll
                for (int j = i + 1; j < NE; ++j) {
                    const float dmin = (i < N ? half_agent : half_obst) + (j < N ? half_agent : half_obst);
                    const float cut = dmin + 18.0f * k_margin;
                    const float dx = p[i].x - p[j].x, dy = p[i].y - p[j].y;
                    const float d2 = dx * dx + dy * dy;
                    if (d2 < cut * cut) {
                        const float d = __builtin_amdgcn_sqrtf(d2);
                        const float x = (dmin - d) / k_margin;
                        const float pen = k_margin * (fmaxf(x, 0.0f) + __logf(1.0f + __expf(-fabsf(x))));
                        const float c = a.p.contact_force * pen * __builtin_amdgcn_rcpf(d);
                        fx[i] += dx * c; fy[i] += dy * c;
                        const float ex = -dx, ey = -dy;                 // p_j - p_i, exactly
                        fx[j] += ex * c; fy[j] += ey * c;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const float2 fa = action_force(a.p, agent_props_of(a.p, i, false), u_now[i], (uint32_t)(b + a.p.env_index_base),
                                               (uint32_t)i, off);
                fx[i] += fa.x; fy[i] += fa.y;
            }
            if (a.p.num_walls > 0) {                    // (one uniform branch around all entities)
#pragma unroll
                for (int i = 0; i < NE; ++i) wall_forces(a.p, p[i], i < N ? half_agent : half_obst, fx[i], fy[i]);
            }
#pragma unroll
            for (int i = 0; i < NE; ++i) {
                v[i].x = v[i].x * (1.0f - a.p.damping) + (fx[i] / a.p.mass) * a.p.dt;
                v[i].y = v[i].y * (1.0f - a.p.damping) + (fy[i] / a.p.mass) * a.p.dt;
                if (i < N) v[i] = clamp_speed(a.p.max_speed, v[i]);
                p[i].x += v[i].x * a.p.dt; p[i].y += v[i].y * a.p.dt;
                if (i >= N) {                           // the reward callback re-arms the obstacle velocity every step (:84-89)
                    const bool falling = p[i].y > a.sc.obstacle_floor;
                    v[i] = make_float2(falling ? a.sc.obstacle_vx : 0.f, falling ? a.sc.obstacle_vy : 0.f);
                }
            }
            t_step += 1;
        }
        // ---- formation term ----
        float form;
        if constexpr (BASIC) {
            float slot[G];
#pragma unroll
            for (int g = 0; g < G; ++g) slot[g] = 0.f;
#pragma unroll
            for (int l = 0; l < L; ++l) {
                float best = INFINITY; int barg = 0;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const float dx = p[j].x - lm[l].x, dy = p[j].y - lm[l].y, d2 = dx * dx + dy * dy;
                    if (d2 < best) { best = d2; barg = j; }
                }
                slot[l % G] += sqrtf(best);
                if (a.near_ag && live) a.near_ag[(kb + b) * L + l] = barg;
            }
            form = lane_group_sum<G>(slot);
        } else {
            float sx[G], sy[G], tx[G], ty[G];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                sx[g] = g < N ? p[g < N ? g : 0].x : 0.f; sy[g] = g < N ? p[g < N ? g : 0].y : 0.f;
                tx[g] = 0.f; ty[g] = 0.f;
            }
#pragma unroll
            for (int l = 0; l < L; ++l) { tx[l % G] += lm[l].x; ty[l % G] += lm[l].y; }
            const float mx = lane_group_sum<G>(sx) * a.inv_n, my = lane_group_sum<G>(sy) * a.inv_n;
            const float lx = lane_group_sum<G>(tx) * a.inv_l, ly = lane_group_sum<G>(ty) * a.inv_l;
            float rowmax = -INFINITY, colmax = -INFINITY;
#pragma unroll
            for (int i = 0; i < N; ++i) {                       // min over landmarks for agent i
                float rowmin = INFINITY;
#pragma unroll
                for (int l = 0; l < L; ++l) {
                    const float dx = (p[i].x - mx) - (lm[l].x - lx), dy = (p[i].y - my) - (lm[l].y - ly);
                    rowmin = fminf(rowmin, dx * dx + dy * dy);
                }
                rowmax = fmaxf(rowmax, rowmin);
            }
#pragma unroll
            for (int l = 0; l < L; ++l) {                       // min over agents for landmark l
                float cm = INFINITY;
#pragma unroll
                for (int j = 0; j < N; ++j) {
                    const float dx = (p[j].x - mx) - (lm[l].x - lx), dy = (p[j].y - my) - (lm[l].y - ly);
                    cm = fminf(cm, dx * dx + dy * dy);
                }
                colmax = fmaxf(colmax, cm);
            }
            form = sqrtf(fmaxf(rowmax, colmax));
        }
        // ---- collision counts (pairs shared: |p_j - p_i|^2 is the same number from either side) ----
        int cnt[N];
#pragma unroll
        for (int i = 0; i < N; ++i) cnt[i] = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            if constexpr (BASIC) {                                      // the self pair (basic_formation_env.py:49-51): distance 0,
                const float dx = p[i].x - p[i].x, dy = p[i].y - p[i].y; //   NaN for a NaN position, as scn_kernel computes it
                cnt[i] += (dx * dx + dy * dy < thr2) ? 1 : 0;
            }
#pragma unroll
            for (int j = i + 1; j < N; ++j) {
                const float dx = p[j].x - p[i].x, dy = p[j].y - p[i].y;
                const int hit = (dx * dx + dy * dy < thr2) ? 1 : 0;
                cnt[i] += hit; cnt[j] += hit;
            }
#pragma unroll
            for (int k = 0; k < M; ++k) {
                const float dx = p[N + k].x - p[i].x, dy = p[N + k].y - p[i].y;
                cnt[i] += (dx * dx + dy * dy < ot2) ? 1 : 0;
            }
        }
        int total = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) total += cnt[i];
        const bool is_done = t_step >= a.p.world_length;
        const float shared = (float)(-(double)N * (double)form - (double)a.sc.penalty * (double)(float)total);
        float indiv[N];
#pragma unroll
        for (int i = 0; i < N; ++i) indiv[i] = -form - a.sc.penalty * (float)cnt[i];
        const uint32_t done_flag = is_done ? 1u : 0u;       // the finished step's flag: the reset below does not change it
        if (a.p.auto_reset && a.do_phys && is_done) {
            // the vec-env worker's rule (env_wrappers.py:14-18): the env restarts at once, the RESET observation goes out
            // with the finished step's reward / done.  The draws fg_reset_scenario makes.
#pragma unroll
            for (int i = 0; i < N; ++i) { p[i] = scn_fresh_pm1(a.p, b, (uint32_t)i, off); v[i] = make_float2(0.f, 0.f); }
#pragma unroll
            for (int k = 0; k < M; ++k) {
                p[N + k] = scn_fresh_obstacle(a.p, b, k, a.sc.num_obstacles, off);
                v[N + k] = make_float2(a.sc.obstacle_vx, a.sc.obstacle_vy);
            }
#pragma unroll
            for (int l = 0; l < L; ++l) lm[l] = scn_fresh_pm1(a.p, b, SCN_LANDMARK_CODE | (uint32_t)l, off);
            fresh_lm = true;
            t_step = 0;
        }
