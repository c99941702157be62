// fg_actor_mlp_preload.inc - the shared actor's small parameters into LDS: wsm = b1 [H] | b2 [H] | W3 [2][H] | b3 [2] |
// (SAMPLE) log_std [2].  Included once at the top of fg_actor_rollout_body.inc (PER_AGENT = false) and of
// fg_scn_lane_actor_body.inc, whose scope provides `w` (ActorW), `log_std`, `wsm`, `tid`, H, WS (= 4 H) and `constexpr bool
// SAMPLE`; both kernels have FG_ACTOR_THREADS threads.  The workgroup barrier before the first actor pass publishes it.
// fg_actor_mlp.inc and the bodies' layer 1 (actor_bias_init) read it back.  Not a header: no guard.
// `constexpr bool LNORM` (with `nw`, ActorNormW): the two hidden LayerNorms' gamma1 [H] | beta1 [H] | gamma2 [H] | beta2 [H]
// follow at wsm + WS + WB (WB: the floats of the b3 | log_std slot, 4), a NULL gamma as ones and a NULL beta as zeros.
// `constexpr bool CAT` or `GUM` - a head of five - (WS = 7 H, WB = 8): W3 [5][H] at wsm + 2 H and b3 [5] at wsm + WS; no log_std.
    for (int q = tid; q < H; q += FG_ACTOR_THREADS) {
        wsm[q] = w.b1 ? w.b1[q] : 0.f;
        wsm[H + q] = w.b2 ? w.b2[q] : 0.f;
        wsm[2 * H + q] = w.w3[q];
        wsm[3 * H + q] = w.w3[H + q];
        if constexpr (CAT || GUM) {
#pragma unroll
            for (int j = 2; j < FG_CAT; ++j) wsm[(2 + j) * H + q] = w.w3[j * H + q];
        }
    }
    if constexpr (CAT || GUM) {
        if (tid < FG_CAT) wsm[WS + tid] = w.b3 ? w.b3[tid] : 0.f;
    } else {
        if (tid < 2) wsm[4 * H + tid] = w.b3 ? w.b3[tid] : 0.f;
    }
    if constexpr (SAMPLE) {
        if (tid < 2) wsm[WS + 2 + tid] = log_std[tid];
    }
    if constexpr (LNORM) {
        float* const lnp = wsm + WS + WB;
        for (int q = tid; q < H; q += FG_ACTOR_THREADS) {
            lnp[q] = nw.g1 ? nw.g1[q] : 1.f;
            lnp[H + q] = nw.be1 ? nw.be1[q] : 0.f;
            lnp[2 * H + q] = nw.g2 ? nw.g2[q] : 1.f;
            lnp[3 * H + q] = nw.be2 ? nw.be2[q] : 0.f;
        }
    }
