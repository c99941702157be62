// fg_scn_lane_write.inc - one hand-over block of a one-env-per-lane workgroup -> global memory: the step body of
// lane_writer_wave (fg_scn_lane_kernel.hpp), shared with scn_lane_actor (fg_scn_lane_actor_kernel.hpp).  Included inside the
// step loop, whose scope provides: smem_all, DB, BLOCK_UNITS, ENVS, U, SU, N, D, NWW, PW (constants), ks, B, b0, El, obs_every,
// obs, rew, indiv, done, lane and the writer wave's index w.  Not a header: no guard.  A textual include for the reason
// written at the top of fg_actor_rollout_body.inc: scn_lane_kernel's ISA stays what it was.
        const float2* const smem = smem_all + (DB ? (ks & 1) * BLOCK_UNITS : 0);
        const float* const s_rew = reinterpret_cast<const float*>(smem + ENVS * SU);
        const float* const s_ind = s_rew + ENVS * N;
        const uint32_t* const s_done = reinterpret_cast<const uint32_t*>(s_ind + ENVS * N);
        const size_t kb = (size_t)ks * B;
        const bool want_obs = obs != nullptr && (obs_every <= 1 || (ks + 1) % obs_every == 0);
        if (want_obs) {
            // unit q of the workgroup's span = unit (q mod U) of env (q div U); 64 units per instruction, lanes consecutive
            const size_t ob = (size_t)(obs_every > 1 ? ks / obs_every : ks) * B;
            float2* const out = reinterpret_cast<float2*>(obs + (ob + (size_t)b0) * N * D);
            if (El == ENVS) {
                // a full block: 32 U pairs of units, one 16-byte store per lane and instruction (1 KiB per wave instruction; the
                // two units of a pair may sit in different rows of the LDS image.  8-byte stores: basic 3.2-3.45 -> 3.1 us/step,
                // partial 6.8-7.5 -> 6.5, profiles/r04_lane_x4_ab.txt).  An odd U makes the image contiguous (pitch U | 1 = U):
                // the pair is ONE 16-byte LDS read, lanes consecutive, no bank conflicts (the two 8-byte reads at a 16-byte lane
                // stride met two-way: SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.21 in profiles/r04_scn_pmc.txt).
                constexpr int NP2 = ENVS / 2 * U, IT = (NP2 + 63) / 64;
                constexpr int MINE = (IT + NWW - 1) / NWW;          // store instructions of one writer wave
                f32x4* const out4 = reinterpret_cast<f32x4*>(out);
                const f32x4* const img4 = reinterpret_cast<const f32x4*>(smem);
#pragma unroll
                for (int t0 = 0; t0 < MINE; t0 += 8) {
                    f32x4 r[8];
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        if (t0 + c < MINE) {
                            const int pair = (w + NWW * (t0 + c)) * 64 + lane;
                            const bool ok = pair < NP2;
                            if constexpr (SU == U) {
                                r[c] = img4[ok ? pair : 0];
                            } else {
                                const int q = 2 * pair;
                                const int r0 = q / U, c0 = q - r0 * U;
                                int r1 = r0, c1 = c0 + 1;
                                if (c1 == U) { c1 = 0; r1 += 1; }
                                const float2 x0 = smem[ok ? r0 * SU + c0 : 0], x1 = smem[ok ? r1 * SU + c1 : 0];
                                r[c] = (f32x4){x0.x, x0.y, x1.x, x1.y};
                            }
                        }
                    }
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const int pair = (w + NWW * (t0 + c)) * 64 + lane;
                        if (t0 + c < MINE && pair < NP2) out4[pair] = r[c];
                    }
                }
            } else {
                const int units = El * U;
                for (int q = w * 64 + lane; q < units; q += 64 * NWW) {
                    const int row = q / U, col = q - row * U;
                    out[q] = smem[row * SU + col];
                }
            }
        }
        // reward, individual reward, done of the 64 x N agents: [K][B][N], the workgroup's slice is contiguous; the 3 N store
        // instructions are dealt over the writer waves
        const int cnt = El * N;
        const size_t o0 = (kb + b0) * N + lane;
        if (rew) {                                  // (one uniform branch per array, not per store)
#pragma unroll
            for (int c = 0; c < N * PW; ++c) if (c % NWW == w && c * 64 + lane < cnt) rew[o0 + c * 64] = s_rew[c * 64 + lane];
        }
        if (indiv) {
#pragma unroll
            for (int c = 0; c < N * PW; ++c) if ((c + 1) % NWW == w && c * 64 + lane < cnt) indiv[o0 + c * 64] = s_ind[c * 64 + lane];
        }
        if (done) {
#pragma unroll
            for (int c = 0; c < N * PW; ++c) if ((c + 2) % NWW == w && c * 64 + lane < cnt) done[o0 + c * 64] = (uint8_t)s_done[c * 64 + lane];
        }
