// fg_scn_lane_actor_kernel.hpp - Closed-loop K-step rollout of the landmark scenarios at their reference shapes, driven by the
// caller's MLP actor (fg_rollout_scenario_actor).  Part of libformation_hip (gfx950); included by formation_hip.hip.
//
// The loop `a = actor(o); o, r, d, info = env.step(a)`, K times in ONE launch, for basic_formation_env,
// formation_hd_partial_env, formation_hd_partial_range_env and formation_hd_obs_env at the seven shapes scn_lane_kernel is
// instantiated for, with the actor
//     Linear(D, H) - ReLU - Linear(H, H) - ReLU - Linear(H, 2) [- Tanh],    D = scn_obs_dim(...), H in {32, 64}
// shared by every agent and read in place from the caller's fp32 parameter tensors (ActorW, fg_actor_rollout_kernel.hpp).
//
// Geometry (one per instantiation, no fill rules): 256 threads = 64 environments per workgroup.  Each step, two phases
// separated by workgroup barriers:
//   producer  wave 0, one env per lane: the step of scn_lane_kernel's producer - the SAME source text (fg_scn_lane_step.inc,
//             fg_scn_lane_compose.inc), so replaying the recorded actions through fg_rollout_scenario gives the same bits - with
//             the action taken from LDS; it composes the env's [N][D] observation block in LDS EVERY step, because the block
//             is the actor's input whether or not obs_every stores it.  Waves 1-3 wait at the barrier.
//   stream +  all four waves store the step's block (fg_scn_lane_write.inc: observations on the obs_every steps, rewards,
//   actor     individual rewards, done flags), then evaluate the MLP for the next step on the block's 64 N rows, 32 rows per wave
//             pass (two 16-row tiles sharing every weight fragment) with the formation_hd_env body's own text after layer 1
//             (fg_actor_mlp.inc; the preload of the small parameters is fg_actor_mlp_preload.inc): layers 1 and 2 on
//             v_mfma_f32_16x16x4_f32 (exact fp32, k ascending, one accumulator chain per output element, bias as the
//             accumulator's initial value), the A operand of layer 1 straight from the block (row r of env e starts at float
//             2 SU e + D r: the odd float2 pitch SU is per env, rows inside an env are contiguous), K = D padded to a multiple
//             of 4 with zero operands, communication columns read like any other; the weights as the B operand from global
//             memory (L2 / L1 hits); layer 3 an ascending fmaf chain on the VALU, one lane per (row, output).  The actions go
//             to LDS for the producer and, from the same lanes, to act_out [K][B][N][2] (256 contiguous bytes per wave pass).
// One producer wave of four leaves three SIMDs idle during the physics, and 64 envs per workgroup leave a 4096-env batch on 64
// of the 256 CUs: accepted, measured in profiles/actor_landmark.md.
// No atomics: two launches from the same state and weights give the same bits.
//
// scn_lane_actor_gauss<...> is the same body with actor_sample_kernel's Gaussian: each lane (row, o) of layer 3 adds
// exp(log_std[o]) * eps[o], eps = actor_eps(seed, global env, agent, offset of the step that takes the action), and the row's
// log-density goes to logp [K][B][N].
#ifndef FG_SCN_LANE_ACTOR_KERNEL_HPP_
#define FG_SCN_LANE_ACTOR_KERNEL_HPP_

#include "fg_scn_lane_kernel.hpp"
#include "fg_actor_rollout_kernel.hpp"

namespace fg {

constexpr int FG_SCN_ACTOR_THREADS = 256;
constexpr int FG_SCN_ACTOR_ENVS = 64;         // one producer wave, one env per lane
static_assert(FG_SCN_ACTOR_THREADS == FG_ACTOR_THREADS, "fg_actor_mlp_preload.inc strides by FG_ACTOR_THREADS");
// LDS (floats): the hand-over block of scn_lane_kernel (observations [64][SU] float2 | reward | individual reward | done, each
//               [64 N]) | actions [64 N][2] | (SAMPLE: log-probs [64 N]) | b1 [H] b2 [H] W3 [2][H] b3 [2] log_std [2] |
//               activations [4][32][H + 4]
__host__ __device__ constexpr int scn_actor_lds_bytes(int kind, int n, int l, int m, int nbr, int h, bool sample) {
    return scn_lane_block_bytes(kind, n, l, m, nbr, 1) +
           ((sample ? 3 : 2) * FG_SCN_ACTOR_ENVS * n + 4 * h + 4 +
            (FG_SCN_ACTOR_THREADS / 64) * FG_ACTOR_ROWS * actor_hstride(h)) * (int)sizeof(float);
}

// SAMPLE = false: the deterministic actor.
template <int KIND, int N, int L, int M, int NBR, int H>
__global__ __launch_bounds__(FG_SCN_ACTOR_THREADS) void scn_lane_actor(const ScnArgs a, const ActorW w, float* act_out) {
    constexpr bool SAMPLE = false;
    const float* const log_std = nullptr;
    float* const logp = nullptr;
#include "fg_scn_lane_actor_body.inc"
}

// SAMPLE = true: the Gaussian actor, log_std [2] read in place, log-probs to logp [K][B][N] when it is not NULL.
template <int KIND, int N, int L, int M, int NBR, int H>
__global__ __launch_bounds__(FG_SCN_ACTOR_THREADS) void scn_lane_actor_gauss(const ScnArgs a, const ActorW w, float* act_out,
                                                                               const float* log_std, float* logp) {
    constexpr bool SAMPLE = true;
#include "fg_scn_lane_actor_body.inc"
}

}  // namespace fg

#endif  // FG_SCN_LANE_ACTOR_KERNEL_HPP_
