// fg_scn_lane_compose.inc - the lane's [N][D] observation block into LDS (scn_lane_kernel's hand-over, shared with
// scn_lane_actor, where the block is also the actor's input).  The including scope provides: a, KIND, N, L, M, NBR, D, SU, BASIC,
// the lane's state p, v, lm, its slot, the block `smem` and `want_obs`.  Not a header: no guard.
        if (want_obs) {
            float2* const mine = smem + slot * SU;
            const float r = (KIND == FG_SCN_RANGE) ? a.sc.obs_range : INFINITY;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                float2* const o = mine + i * (D / 2);
                int w = 0;
                o[w++] = v[i];
                if constexpr (BASIC) o[w++] = p[i];
#pragma unroll
                for (int l = 0; l < L; ++l) o[w++] = BASIC ? make_float2(lm[l].x - p[i].x, lm[l].y - p[i].y) : lm[l];
#pragma unroll
                for (int k = 0; k < M; ++k) o[w++] = make_float2(p[N + k].x - p[i].x, p[N + k].y - p[i].y);
                if constexpr (KIND == FG_SCN_PARTIAL) {
#pragma unroll
                    for (int kk = 0; kk < NBR; ++kk) {
                        int j = i + 1 + kk;                             // (i + 1 + kk) mod N
                        while (j >= N) j -= N;
                        o[w++] = make_float2(p[j].x - p[i].x, p[j].y - p[i].y);
                    }
                } else {
#pragma unroll
                    for (int t = 0; t < N - 1; ++t) {
                        const int j = t < i ? t : t + 1;                // the t-th OTHER agent, index order
                        o[w++] = make_float2(fminf(fmaxf(p[j].x - p[i].x, -r), r), fminf(fmaxf(p[j].y - p[i].y, -r), r));
                    }
                }
#pragma unroll
                for (int t = 0; t < N - 1; ++t) o[w++] = make_float2(0.f, 0.f);
            }
        }
