// fg_actor_mlp.inc - the MLP core of the fused actor rollouts: everything a wave pass of FG_ACTOR_ROWS rows does after layer 1
// for the shared actor `w` - ReLU hand-over, layer 2 on the MFMA with its three WaveSync points, layer 3 and the tanh on the
// VALU, the Gaussian step.  The one copy for fg_actor_rollout_body.inc (formation_hd_env, PER_AGENT = false) and
// fg_scn_lane_actor_body.inc (landmark scenarios); layer 1 stays with each body, whose A operand differs.  Included inside the
// pass loop of the body's `actor` lambda, right after its layer 1 (a textual include for the reason written at the top of
// fg_actor_rollout_body.inc: as a lambda this text changed the kernels' instructions).  Not a header: no guard.
//
// The including scope provides: `acc` (layer 1's accumulators, bias included), `hb` (the wave's activation tile), `wsm` (the
// LDS block fg_actor_mlp_preload.inc fills) and WS, `w`, `a` (a.p: KParams), `lane`, `col`, `kq`, `q0` (the pass's first row),
// `b0` (the workgroup's first env), `off` (the counter offset of the step that takes the action), N, H, HS, CB, RT, SAMPLE.
// It leaves in scope: `row`, `o` (the lane's row of the pass and output), `q` = q0 + row (env-major row of the workgroup:
// env q / N, agent q % N), `y` (the lane's action component, noise added) and, SAMPLE only, the row's draw `n` with `ls0`,
// `ls1` for gauss_logp(n, ls0, ls1).  The body stores them - each to its own place - and ends the pass with a WaveSync.
// `constexpr bool LNORM` (with `nw`): a LayerNorm over each row of the tile after either ReLU hand-over (actor_row_norm on
// gamma | beta at wsm + WS + WB, fg_actor_mlp_preload.inc), with a WaveSync of its own before the next layer reads the tile.
// `constexpr bool GRU` (with `gw`, `gsm`, `hst`; formation_hd_env's body only): the recurrent layer on the tile between the
// second hidden norm and layer 3 (fg_actor_gru.inc), which leaves LayerNorm(h') in the tile for layer 3.
// `constexpr bool OU` (with `ow`, `oust`, `El`; formation_hd_env's body only): the row's noise state at oust + 2 q steps with
// the row's draw (ou_step) and `y` becomes clamp(y + scale x, -clip, clip) (ou_action).
// `constexpr bool CAT` (with `cw`; formation_hd_env's body only): layer 3 has five outputs, W3 [5][H] at wsm + 2 H and b3 [5] at
// wsm + WS.  Both lanes of a row evaluate the five ascending chains (the same bits), draw the row's uniform at `off` and run
// cat_pick (cw.greedy: the mode instead of a sample, wave-uniform); `y` is component o of the decoded action (cat_decode by
// cw.mode) and `pick` the row's index and log-prob, which the body stores.  No tanh.
// `constexpr bool GUM` (with `gum`, ActorGumW; formation_hd_env's body only): the same five-logit block, then the row's five
// Gumbel draws at `off` (actor_gumbel; none when gum.explore is 0, wave-uniform) and gumbel_pick; `y` is component o of the decoded
// action (cat_decode by gum.mode) and `pick.idx` the row's index, which the body stores.  No log-prob, no tanh.
            actor_store_tile(hb, HS, acc, col, kq);
            WaveSync()();
            if constexpr (LNORM) {
                actor_row_norm<H>(hb, HS, wsm + WS + WB, nw.eps1, lane);
                WaveSync()();
            }
            // ---- layer 2 ----
            actor_bias_init(acc, wsm + H, col);
            // (opaque per pass: the weight fragments do not depend on the tile, and hoisted out of the tile loop they would
            // all be held in registers)
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
            WaveSync()();                          // every read of the layer-1 tile before it is overwritten
            actor_store_tile(hb, HS, acc, col, kq);
            WaveSync()();
            if constexpr (LNORM) {
                actor_row_norm<H>(hb, HS, wsm + WS + WB + 2 * H, nw.eps2, lane);
                WaveSync()();
            }
            if constexpr (GRU) {
#include "fg_actor_gru.inc"
            }
            // ---- layer 3 on the VALU: lane = (row of the pass, output), an ascending fmaf chain ----
            const int row = lane >> 1, o = lane & 1;
            const float* const hr = hb + row * HS;
            const float* const w3 = wsm + 2 * H + ((CAT || GUM) ? 0 : o * H);
            float y = (CAT || GUM) ? 0.f : wsm[4 * H + o];
            CatPick pick = {};                     // CAT: the row's index and log-prob; GUM: the row's index
            if constexpr (CAT || GUM) {
                float l[FG_CAT];
#pragma unroll
                for (int j = 0; j < FG_CAT; ++j) l[j] = wsm[WS + j];
#pragma unroll 4
                for (int k = 0; k < H; ++k) {
                    const float hk = hr[k];
#pragma unroll
                    for (int j = 0; j < FG_CAT; ++j) l[j] = __builtin_fmaf(hk, w3[j * H + k], l[j]);
                }
                const int qc = q0 + row, ee = qc / N;
                if constexpr (GUM) {
                    // both lanes of a row draw the row's five Gumbel values at counter offset `off` and pick the same index
                    float gd[FG_CAT] = {};
                    if (gum.explore) actor_gumbel(a.p.seed, (uint32_t)(b0 + ee + a.p.env_index_base), (uint32_t)(qc - ee * N), off, gd);
                    pick.idx = gumbel_pick(l, gd, gum.explore != 0);
                    const float2 ua = cat_decode(gum.mode, pick.idx);
                    y = o ? ua.y : ua.x;
                } else {
                // both lanes of a row draw the row's uniform at counter offset `off` and pick the same index
                const float ud = cw.greedy ? 0.f
                                           : actor_uniform(a.p.seed, (uint32_t)(b0 + ee + a.p.env_index_base), (uint32_t)(qc - ee * N), off);
                pick = cat_pick(l, ud, cw.greedy != 0);
                const float2 ua = cat_decode(cw.mode, pick.idx);
                y = o ? ua.y : ua.x;
                }
            } else {
#pragma unroll 8
                for (int k = 0; k < H; ++k) y = __builtin_fmaf(hr[k], w3[k], y);
                if (w.out_tanh) y = tanhf(y);
            }
            // the pass's row as an env-major row of the workgroup: env q / N, agent q % N
            const int q = q0 + row;
            float2 n = {};                         // SAMPLE: the row's draw and log_std, for gauss_logp(n, ls0, ls1)
            float ls0 = 0.f, ls1 = 0.f;
            if constexpr (SAMPLE) {
                const int ee = q / N;
                // both lanes of a row draw the row's pair at counter offset `off`: lane o adds component o
                n = actor_eps(a.p.seed, (uint32_t)(b0 + ee + a.p.env_index_base), (uint32_t)(q - ee * N), off);
                ls0 = wsm[WS + 2]; ls1 = wsm[WS + 3];
                y += __expf(o ? ls1 : ls0) * (o ? n.y : n.x);
            }
            if constexpr (OU) {
                const int ee = q / N;
                // the Gaussian kernels' draw of (env, agent) at `off`; lane o steps component o of its own row's state
                n = actor_eps(a.p.seed, (uint32_t)(b0 + ee + a.p.env_index_base), (uint32_t)(q - ee * N), off);
                if (q < El * N) {
                    const float x = ou_step(oust[2 * q + o], o ? n.y : n.x, ow.theta, ow.mu, ow.sigma);
                    oust[2 * q + o] = x;
                    y = ou_action(y, x, ow.scale, ow.clip);
                }
            }
