// fg_actor_gru.inc - the recurrent layer of gru_actor_kernel / gru_sample_kernel: one torch.nn.GRUCell step on a wave pass of
// FG_ACTOR_ROWS rows, then the LayerNorm that follows it.  Included by fg_actor_mlp.inc under `if constexpr (GRU)`, after the
// second hidden norm has left x in the wave's tile `hb` and before layer 3, which then reads LayerNorm(h') from the same tile.
// (A textual include for the reason written at the top of fg_actor_rollout_body.inc.)  Not a header: no guard.
//
// The including scope provides, beside fg_actor_mlp.inc's own list: `gw` (ActorGruW), `gsm` (the LDS block b_ir + b_hr |
// b_iz + b_hz | b_in | b_hn | gamma3 | beta3 the body fills) and `hst` (the workgroup's hidden state, row q at hst + q HS;
// rows q0 .. q0 + FG_ACTOR_ROWS - 1 are this pass's and this wave's alone).
//     r = sigmoid(W_ir x + W_hr h + (b_ir + b_hr))      acc
//     z = sigmoid(W_iz x + W_hz h + (b_iz + b_hz))      az
//     n = tanh((W_in x + b_in) + r (W_hn h + b_hn))     an, ahn
//     h' = (1 - z) n + z h
// Each product is layer 2's: v_mfma_f32_16x16x4_f32 over ascending k, the weights as the B operand from global memory (three
// gates' fragments per k chunk and column block), x / h as the A operand from LDS.  The gates are element-wise in the
// accumulator layout (register j of lane l: row 4 (l >> 4) + j, column l & 15 of its tile), where h is read back and h' written
// to the state and, for the norm and layer 3, over x in the tile.  Also from the including scope: `off` and `rbase` (the step
// is off - rbase), `M` (the workgroup's live rows) and `b0`, for the record of the states below.
                float* const hs = hst + q0 * HS;
                // The record of the states (gw.states, wave-uniform): hs is the state this step acts with - the physics phase
                // has zeroed the rows whose last step ended an episode, a workgroup barrier ago - and these rows are this wave's
                // alone, so the wave stores them itself, before the products, with no barrier of its own.  The pass's rows are one
                // span of FG_ACTOR_ROWS H floats of entry kstep / states_every, 16 bytes per lane and store (rows stay 16-byte
                // aligned at the pitch H + 4); rows past the workgroup's agents - a tail workgroup's, the last tile's padding - are
                // not stored.
                if (gw.states != nullptr) {
                    static_assert(HS % 4 == 0 && (FG_ACTOR_ROWS * H / 4) % 64 == 0, "the state's rows are read 16 bytes at a time");
                    const int kstep = (int)(off - rbase);
                    if (kstep % gw.states_every == 0) {
                        float* const dst = gw.states + (((size_t)(kstep / gw.states_every) * a.B + b0) * N + q0) * H;
#pragma unroll
                        for (int it = 0; it < FG_ACTOR_ROWS * H / 256; ++it) {
                            const int idx = it * 64 + lane, srow = idx / (H / 4), c4 = idx % (H / 4);
                            if (q0 + srow < M)
                                reinterpret_cast<float4*>(dst)[idx] = *reinterpret_cast<const float4*>(hs + srow * HS + 4 * c4);
                        }
                    }
                }
                f32x4 az[RT][CB], an[RT][CB], ahn[RT][CB];
                actor_bias_init(acc, gsm, col);
                actor_bias_init(az, gsm + H, col);
                actor_bias_init(an, gsm + 2 * H, col);
                actor_bias_init(ahn, gsm + 3 * H, col);
                // (opaque per pass, as layer 2's)
                const float* wih = gw.w_ih + (size_t)col * H;
                const float* whh = gw.w_hh + (size_t)col * H;
                asm volatile("" : "+v"(wih));
                asm volatile("" : "+v"(whh));
#pragma unroll 2
                for (int ks = 0; ks < H / 4; ++ks) {   // the input's three products
                    const int k = ks * 4 + kq;
                    float xa[RT];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) xa[rt] = hb[(rt * 16 + col) * HS + k];
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb) {
                        const float wr = wih[cb * 16 * H + k], wz = wih[(H + cb * 16) * H + k], wn = wih[(2 * H + cb * 16) * H + k];
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) {
                            acc[rt][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[rt], wr, acc[rt][cb], 0, 0, 0);
                            az[rt][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[rt], wz, az[rt][cb], 0, 0, 0);
                            an[rt][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[rt], wn, an[rt][cb], 0, 0, 0);
                        }
                    }
                }
#pragma unroll 2
                for (int ks = 0; ks < H / 4; ++ks) {   // the state's three products
                    const int k = ks * 4 + kq;
                    float ha[RT];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) ha[rt] = hs[(rt * 16 + col) * HS + k];
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb) {
                        const float wr = whh[cb * 16 * H + k], wz = whh[(H + cb * 16) * H + k], wn = whh[(2 * H + cb * 16) * H + k];
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) {
                            acc[rt][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[rt], wr, acc[rt][cb], 0, 0, 0);
                            az[rt][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[rt], wz, az[rt][cb], 0, 0, 0);
                            ahn[rt][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ha[rt], wn, ahn[rt][cb], 0, 0, 0);
                        }
                    }
                }
                WaveSync()();                          // every read of x and of h as an operand before either is overwritten
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int cb = 0; cb < CB; ++cb)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int at = (rt * 16 + kq * 4 + j) * HS + cb * 16 + col;
                            const float r = 1.0f / (1.0f + expf(-acc[rt][cb][j]));
                            const float z = 1.0f / (1.0f + expf(-az[rt][cb][j]));
                            const float n = tanhf(__builtin_fmaf(r, ahn[rt][cb][j], an[rt][cb][j]));
                            const float hn = __builtin_fmaf(z, hs[at] - n, n);     // (1 - z) n + z h
                            hs[at] = hn;
                            hb[at] = hn;
                        }
                WaveSync()();
                actor_row_norm<H>(hb, HS, gsm + 4 * H, gw.eps3, lane);
                WaveSync()();
