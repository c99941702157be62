// fg_actor_rollout_kernel.hpp - Closed-loop K-step rollout driven by the caller's MLP actor (fg_rollout_hd_actor).
// Part of libformation_hip (gfx950); included by formation_hip.hip.
//
// The loop of a learned actor, `a = actor(o); o, r, d, info = env.step(a)`, K times in ONE launch, with the actor
//     Linear(6N, H) - ReLU - Linear(H, H) - ReLU - Linear(H, 2) [- Tanh]
// shared by every agent (parameter sharing) and read in place from the caller's fp32 parameter tensors (torch Linear
// layout [out][in]; NULL biases are zero).
//
// Geometry (one per (N, H), no fill rules): 256 threads, G = N rounded up to a power of two (>= 4) lanes per env, E = 256 / G
// envs per workgroup.  Each step, in three phases separated by workgroup barriers:
//   physics  every lane runs World.step + reward + auto-reset of its agent with the device functions of rollout_kernel
//            (fg_pair_loops.hpp, the butterflies of fg_common.hpp, the same Philox counters) in the same order, so replaying
//            the recorded actions through fg_rollout_hd gives the same bits; it publishes the env's observation tables
//   stream   the four waves store the step's observations from the tables (write_obs_rows, fg_obs_writers.hpp) and then
//   actor    evaluate the MLP for the next step: the rows of the product are the workgroup's E x N agents, taken 32 at a time
//            per wave (two 16-row tiles sharing every weight fragment); layers 1 and 2 on v_mfma_f32_16x16x4_f32 (exact fp32,
//            one rounding per product) with the weights as the B operand straight from global memory (every workgroup reads
//            the same few tens of KiB: L2 / L1 hits), the activations through a per-wave LDS tile; layer 3 (two outputs) on
//            the VALU, one lane per (row, output).  Layer 1 reads its input straight from the tables - the units the
//            observation writers store - and skips the communication block (zero for silent agents).
// No atomics: two launches from the same state and weights give the same bits.
// The actor network after layer 1 (ReLU hand-over, layer 2, layer 3, tanh, Gaussian step) and the LDS preload of b1 | b2 | W3 |
// b3 | log_std are fg_actor_mlp.inc and fg_actor_mlp_preload.inc, the one copy that fg_actor_rollout_body.inc and the landmark
// scenarios' fg_scn_lane_actor_body.inc include; actor_bias_init, actor_store_tile and gauss_logp below are their small pieces.
//
// actor_sample_kernel<N,H> (fg_rollout_hd_actor_sample) is the same body with a state-independent diagonal Gaussian on top of
// the actor's output: each lane (row, o) of layer 3 adds exp(log_std[o]) * eps[o], eps = actor_eps(...) drawn from the
// counter stream of the step that takes the action, and each row's log-density goes out with the action.
//
// pa_actor_kernel<N,H> / pa_sample_kernel<N,H> (fg_rollout_hd_actor_per_agent) are the same body with one actor per agent
// (MADDPG-style): agent i's observation rows go through agent i's parameters.  The actor rows are taken agent-major - agent r
// owns the rows r EP .. r EP + EP - 1, EP = max(E, 16), one per env of the workgroup - so that each 16-row MFMA tile belongs
// to one agent, whose weight base pointers come from the by-value table `ActorTab` in the kernel arguments (wave-uniform
// index: scalar loads).  Biases and W3 are read through L1 instead of LDS (4H + 2 floats per agent, 66 KB at 32 x 128).
// At E = 8 (N > 16) the tiles are half full.  Same instructions in the same k order per output element as the shared
// kernels: N identical members give their bits.
//
// ln_actor_kernel<N,H> / ln_sample_kernel<N,H> (fg_rollout_hd_actor_norm, H in {32, 64}) are the shared-actor body with the
// LayerNorms of onpolicy's MLPBase (the MAPPO trainers' actor):
//     [LayerNorm(6N) -] Linear - ReLU - LayerNorm(H) - Linear - ReLU - LayerNorm(H) - Linear(H, 2) [- Tanh]
// selected by `constexpr bool LNORM` (false in every other kernel, whose instructions it leaves as they were).  Each norm is
// torch's: mean and biased variance of the row in fp32, the variance from the centred values (mean first, then the sum of
// squared deviations), rstd = 1 / sqrt(var + eps), y = (x - mean) rstd gamma + beta; gamma / beta read in place (NULL: 1 / 0).
//   hidden norms  on the wave's 32 x H activation tile in LDS, between actor_store_tile and the next layer's reads
//                 (actor_row_norm): four lanes per row, 16 rows at a time, lane (row, c) holding columns c, c + 4, ... - with
//                 the row pitch H + 4 the 32 lanes of a ds_read_b32 / ds_write_b32 group (8 rows x 4 columns) fall on 32
//                 different banks - the two row sums by DPP quad permutes.
//   input norm    a run-time, wave-uniform fact of the launch (ActorNormW::in_norm).  The row statistics come from the
//                 observation tables over all 6N features, the zero communication block included, summed by the four
//                 lanes (k = lane >> 4) that share a row of the A operand; layer 1 then normalises its A operand on the fly
//                 and runs over the WHOLE k range (a normalised zero is beta - mean rstd gamma, not zero).
// gamma / beta of the three norms sit in LDS behind b3 | log_std (fg_actor_mlp_preload.inc; the input norm's from the body).
//
// gru_actor_kernel<N,H> / gru_sample_kernel<N,H> (fg_rollout_hd_actor_gru, H in {32, 64}) are the LayerNorm body with the
// recurrent layer of onpolicy's R_Actor (rMAPPO's policy, recurrent_N = 1) between the second hidden norm and the head:
//     [LayerNorm(6N) -] Linear - ReLU - LayerNorm(H) - Linear - ReLU - LayerNorm(H) - GRU(H, H) - LayerNorm(H) - Linear(H, 2)
//     [- Tanh]
// selected by `constexpr bool GRU` (false in every other kernel, whose instructions it leaves as they were); the recurrent part
// of a wave pass is fg_actor_gru.inc.  One GRU step per actor evaluation, torch.nn.GRUCell's (gate order r | z | n):
//     r = sigmoid(W_ir x + b_ir + W_hr h + b_hr), z likewise, n = tanh(W_in x + b_in + r (W_hn h + b_hn)), h' = (1 - z) n + z h
// with the six products on v_mfma_f32_16x16x4_f32 - the weights as the B operand read in place, x from the wave's tile and h
// from the state block as A operands - and the gates element-wise in the accumulator layout.  h' is the state carried on; the
// head sees LayerNorm(h').
//   state         every row's h [H] lives in LDS for the whole launch, one block of TILES x 32 rows at the tile's pitch H + 4
//                 behind the activation tiles: loaded from `rnn_state` once at launch start, stored once at the end.  A row
//                 belongs to one wave for the whole launch (tile t is wave t % 4's), so only that wave reads or writes it in
//                 the actor phase; the physics phase zeroes the rows of an env whose step ended its episode (is_done, with
//                 or without auto-reset), a workgroup barrier away from either neighbour.
//   kept states   fg_rollout_hd_actor_gru_states (ActorGruW::states, a run-time, wave-uniform fact of the launch): before the
//                 six products of step k with k % states_every == 0, the wave that owns a tile stores its rows - the state the
//                 step acts with, masking applied - to entry k / states_every of `rnn_states`, 16 bytes per lane and store.
//                 Its own rows only, so no barrier is added; without `states` the pass takes one scalar branch.
//
// bn_actor_kernel<N,H> / bn_sample_kernel<N,H> (fg_rollout_hd_actor_bn) and pa_bn_actor_kernel<N,H> / pa_bn_sample_kernel<N,H>
// (fg_rollout_hd_actor_bn_per_agent), H in {32, 64}, are the shared and the per-agent body behind an eval-mode BatchNorm1d over
// the actor's input (the MADDPG trainers' `in_fn`: running statistics, no batch statistics):
//     BatchNorm1d(6N) - Linear - ReLU - Linear - ReLU - Linear(H, 2) [- Tanh]
// selected by `constexpr bool INBN` (false in every other kernel, whose instructions it leaves as they were).  Per feature k,
// torch's eval-mode arithmetic in one spelling for both bodies (bn_istd, bn_apply), so N identical members give the shared
// kernel's bits:
//     istd_k = 1 / sqrt(var_k + eps),    x'_k = fma((x_k - mean_k) istd_k, gamma_k, beta_k)      (NULL gamma / beta: 1 / 0)
// x' is layer 1's A operand; layer 1 runs over the WHOLE k range as with the input LayerNorm (a normalised zero of the
// communication block is beta - mean istd gamma).  Everything after layer 1 is the plain body's.
//   shared     mean | istd | gamma | beta, each [DP] (DP = 6N rounded up to 4) with zeros at k >= 6N, are filled once per
//              workgroup in LDS behind b3 | log_std, published by the barrier that publishes the preload.
//   per agent  each 16-row tile's agent's four pointers and eps come from the by-value table `ActorBnTab` in the kernel
//              arguments (wave-uniform index: scalar loads); the statistics are read through L1 like the per-agent biases, and
//              istd is recomputed per element (the same two lines of arithmetic).
//
// ou_actor_kernel<N,H>, pa_ou_actor_kernel<N,H>, bn_ou_actor_kernel<N,H> and pa_bn_ou_actor_kernel<N,H> (fg_rollout_hd_actor_ou,
// fg_rollout_hd_actor_ou_per_agent) are the OU member (ACTOR_OU) of the four families without LayerNorms: the deterministic body with
// the MADDPG trainers' exploration on top, selected by `constexpr bool OU` (false in every other kernel, whose instructions it
// leaves as they were).  Per (env, agent) a noise state x [2] is carried from step to step; the step that takes an action does
//     x <- ou_step(x, eps)  =  x + theta (mu - x) + sigma eps,         a = clamp(actor(o) + scale x, -clip, clip)
// (ou_step, ou_action below: the one spelling for every kernel and for the host-paced loop's actor_ou_step_kernel), eps the
// Gaussian kernels' actor_eps at the same counter offsets, clip = +inf for no clamp; there is no log_std and no log-density.
//   state      x lives in LDS for the whole launch, one block [E N][2] behind the activation tiles, indexed by the env-major
//              slot e N + i in the shared and in the agent-major per-agent body alike: loaded from ActorOuW::state at launch
//              start, stored back after the last step.  Lane (row, o) of layer 3 updates component o of its row; a row belongs
//              to one wave for the whole launch, so the actor phase adds no barrier.  The physics phase writes mu into the rows
//              of an env whose step ended its episode (is_done, with or without auto-reset), a workgroup barrier away from
//              either neighbour - the convention of the GRU state's masking.
//
// cat_actor_kernel<N,H>, ln_cat_actor_kernel<N,H> and gru_cat_actor_kernel<N,H> (fg_rollout_hd_actor_cat) are the categorical member
// (ACTOR_CAT) of the plain, LayerNorm and recurrent families: the body with a five-output head under a Categorical (the MAPPO trainers'
// discrete-action policy), selected by `constexpr bool CAT` (false in every other kernel, whose instructions it leaves as they
// were).  W3 [5][H] and b3 [5] sit in LDS where W3 [2][H] | b3 [2] do (fg_actor_mlp_preload.inc).  Both lanes of a row evaluate
// the five logits (ascending fmaf chains from b3[j]: identical bits in both), draw the row's uniform (actor_uniform: word 2 of
// the Gaussian members' Philox block) and run cat_pick; lane o writes component o of the decoded u (cat_decode, by the env's
// action mode) to the actions' block, lane 0 the index and the log-prob to two blocks [E N] behind it, and the physics phase
// stores all three.  ONE kernel per (family, N, H): `greedy` and the action mode are run-time, wave-uniform facts of the launch
// (ActorCatW).  There is no tanh and no log_std.
//
// gumbel_actor_kernel<N,H>, pa_gumbel_actor_kernel<N,H>, bn_gumbel_actor_kernel<N,H> and pa_bn_gumbel_actor_kernel<N,H>
// (fg_rollout_hd_actor_gumbel, fg_rollout_hd_actor_gumbel_per_agent) are the Gumbel member (ACTOR_GUMBEL) of the four families
// without LayerNorms - the OU member's discrete twin: the body with a five-output head whose action is MADDPG's
// gumbel_softmax(logits, hard=True) while exploring and onehot_from_logits(logits) otherwise, selected by `constexpr bool GUM`
// (false in every other kernel, whose instructions it leaves as they were).  The shared families keep W3 [5][H] | b3 [5] in LDS
// as the categorical member does; the per-agent families read the tile's agent's through L1 (ActorTab).  Both lanes of a row
// evaluate the five logits (ascending fmaf chains from b3[j]: identical bits in both), draw the row's five Gumbel values
// (actor_gumbel: a Philox stream of its own, so the Gaussian, OU and categorical draws keep their bits) and run gumbel_pick -
// the lowest index of the largest l_j + g_j, or of the largest l_j when not exploring; lane o writes component o of the decoded
// u (cat_decode, by the env's action mode) to the actions' block and lane 0 the index to the block [E N] behind it, and the
// physics phase stores both.  ONE kernel per (family, N, H): `explore` and the action mode are run-time, wave-uniform facts of
// the launch (ActorGumW).  No temperature (argmax softmax(y / T) = argmax y), no tanh, no log_std, no log-prob.
//
// actor_sample_obs16<N,H>, ln_sample_obs16<N,H>, gru_sample_obs16<N,H>, cat_actor_obs16<N,H>, ln_cat_actor_obs16<N,H> and
// gru_cat_actor_obs16<N,H> (fg_rollout_hd_actor_obs16, fg_rollout_hd_actor_cat_obs16; N in {3, 9, 27}, H in {32, 64}) are the
// Gaussian and the categorical member of the plain, LayerNorm and recurrent families with 16-bit observations (ACTOR_GAUSS16,
// ACTOR_CAT16), selected by
// `constexpr bool OBS16` (false in every other kernel, whose instructions it leaves as they were): the stream phase stores each
// (x, y) unit as one 32-bit word of two fp16 or bf16 halves through write_obs16 (fg_obs_writers.hpp) - the subtractions of
// write_obs_rows on the same table entries, packed round to nearest even: `.to(dtype)` of the fp32 kernel's observations bit for
// bit - and nothing else differs.  ONE kernel per (member, N, H): the format is the last kernel argument, a run-time,
// wave-uniform fact of the launch.  The writer's tile (one per wave, obs16_tile_words words) is the wave's own activation tile:
// only that wave touches either, its stream phase precedes its actor pass in program order, so no barrier and no LDS is added.
// a.obs then holds 32-bit units and a.obs_pitch counts them (3 N^2 per env: a contiguous tensor only).
//
// How the kernels are wired up: a kernel is (family, member).  A member (ActorMember) is stated once, by its predicates below:
// the body's SAMPLE / OU / CAT / OBS16 / GUM and the host's LDS bytes both come from them, and actor_lds_layout is the one statement
// of the LDS blocks.  A family is one block at the end of this file - its kind, its flags, the operands it takes and the ones it
// does not, the names of the members it has - around fg_actor_family.inc, which emits a kernel per named member with
// fg_actor_rollout_body.inc as a textual include, and then HdActorFamily<kind>, the record the host launches from
// (formation_hip.hip: launch_hd_member).  DESIGN.md lists what adding a member or a family takes.
#ifndef FG_ACTOR_ROLLOUT_KERNEL_HPP_
#define FG_ACTOR_ROLLOUT_KERNEL_HPP_

#include "fg_common.hpp"
#include "fg_pair_loops.hpp"
#include "fg_obs_writers.hpp"
#include "fg_policy_kernels.hpp"      // WaveSync

namespace fg {

// the caller's actor as the kernel reads it (FgActor without the hidden width, which is a template parameter)
struct ActorW {
    const float* w1; const float* b1;         // [H][6N], [H]
    const float* w2; const float* b2;         // [H][H],  [H]
    const float* w3; const float* b3;         // [2][H],  [2]
    int out_tanh;
};

// the LayerNorms of ln_*_kernel (FgActorNorm): gamma / beta (NULL: 1 / 0) and eps of the input norm (read only when in_norm)
// and of the two hidden norms
struct ActorNormW {
    const float* g0; const float* be0;        // [6N]
    const float* g1; const float* be1;        // [H]
    const float* g2; const float* be2;        // [H]
    float eps0, eps1, eps2;
    int in_norm;
};

// the recurrent layer of gru_*_kernel (FgActorGru): torch's GRU parameters (gate order r | z | n), the LayerNorm after it
// (gamma / beta NULL: 1 / 0) and the hidden state, read at launch start and written back at the end; `states` (NULL: none
// kept) receives the state every states_every-th step acted with (fg_rollout_hd_actor_gru_states)
struct ActorGruW {
    const float* w_ih; const float* w_hh;     // [3H][H]
    const float* b_ih; const float* b_hh;     // [3H]
    const float* g3; const float* be3;        // [H]
    float eps3;
    float* state;                             // [B][N][H]
    float* states;                            // [ceil(K / states_every)][B][N][H]
    int states_every;
};

// one actor per agent (pa_*_kernel): agent i's parameters; entries at i >= N are never read
constexpr int FG_ACTOR_MAX_AGENTS = 32;
struct ActorTab {
    const float* w1[FG_ACTOR_MAX_AGENTS]; const float* b1[FG_ACTOR_MAX_AGENTS];
    const float* w2[FG_ACTOR_MAX_AGENTS]; const float* b2[FG_ACTOR_MAX_AGENTS];
    const float* w3[FG_ACTOR_MAX_AGENTS]; const float* b3[FG_ACTOR_MAX_AGENTS];
    int out_tanh;
};

// the eval-mode input BatchNorm of bn_*_kernel (FgActorInBn): running mean / variance [6N], gamma / beta (NULL: 1 / 0), eps
struct ActorBnW {
    const float* mean; const float* var;
    const float* gamma; const float* beta;
    float eps;
};
// ... of pa_bn_*_kernel: agent i's; entries at i >= N are never read
struct ActorBnTab {
    const float* mean[FG_ACTOR_MAX_AGENTS]; const float* var[FG_ACTOR_MAX_AGENTS];
    const float* gamma[FG_ACTOR_MAX_AGENTS]; const float* beta[FG_ACTOR_MAX_AGENTS];
    float eps[FG_ACTOR_MAX_AGENTS];
};
// The one spelling of the input BatchNorm's arithmetic (shared and per-agent kernels):
FG_DEV float bn_istd(float var, float eps) { return 1.0f / sqrtf(var + eps); }
FG_DEV float bn_apply(float x, float mean, float istd, float gamma, float beta) {
    return __builtin_fmaf((x - mean) * istd, gamma, beta);
}

// the Ornstein-Uhlenbeck exploration of *ou_actor_kernel (FgActorOu) and the noise state [B][N][2], read at launch start and
// written back at the end
struct ActorOuW {
    float theta, mu, sigma, scale, clip;
    float* state;
};
// The one spelling of the noise state's update, x + theta (mu - x) + sigma eps, per component: three roundings (the
// difference and the two fmas).  theta = 1, mu = 0: fma(1, -x, x) = 0 exactly, so x' = fl(sigma eps) - i.i.d. noise.
FG_DEV float ou_step(float x, float eps, float theta, float mu, float sigma) {
    return __builtin_fmaf(sigma, eps, __builtin_fmaf(theta, mu - x, x));
}
// ... and of the action, clamp(mean + scale x, -clip, clip): a product, then a sum (never contracted), then max / min, which is
// torch's fp32 clamp(mean + scale * x, -clip, clip) bit for bit; clip = +inf leaves the sum as it is.
FG_DEV float ou_action(float mean, float x, float scale, float clip) {
#pragma clang fp contract(off)
    const float noise = scale * x;
    const float v = mean + noise;
    return fminf(fmaxf(v, -clip), clip);
}

// the categorical head of *cat_actor_kernel (fg_rollout_hd_actor_cat): the env's action mode (FG_ACT_ONEHOT5 / FG_ACT_INDEX),
// whether the launch takes the mode of the distribution instead of a sample, and the outputs idx [K][B][N] and logp [K][B][N]
// (NULL: not written)
struct ActorCatW {
    int mode, greedy;
    int* idx;
    float* logp;
};
constexpr int FG_CAT = 5;                     // the five actions of the discrete action space: none, and two per axis

// the Gumbel head of *gumbel_actor_kernel (fg_rollout_hd_actor_gumbel*): the env's action mode (FG_ACT_ONEHOT5 / FG_ACT_INDEX),
// whether the launch explores (argmax of logits + Gumbel noise) or takes the largest logit, and the output idx [K][B][N]
struct ActorGumW {
    int mode, explore;
    int* idx;
};

constexpr int FG_ACTOR_THREADS = 256;
constexpr int FG_ACTOR_ROWS = 32;             // rows of one wave pass: two 16-row MFMA tiles
__host__ __device__ constexpr int actor_lanes(int n) { return n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : 32; }
__host__ __device__ constexpr int actor_envs(int n) { return FG_ACTOR_THREADS / actor_lanes(n); }
__host__ __device__ constexpr int actor_hstride(int h) { return h + 4; }   // row pitch of the activation tile: 16 rows x 4 k conflict-free
__host__ __device__ constexpr int actor_in_pad(int n) { return (6 * n + 3) / 4 * 4; }
__host__ __device__ constexpr int actor_state_rows(int n) {
    return (actor_envs(n) * n + FG_ACTOR_ROWS - 1) / FG_ACTOR_ROWS * FG_ACTOR_ROWS;
}

// A kernel is (family, member).  The family is the network around the MLP - four flags, one value per family block below -
// and the member is what happens to the head's output and to the observations; its four facts are the predicates' answers.
struct ActorFlags { bool per_agent, lnorm, gru, in_bn; };
// Members: the deterministic actor; under a diagonal Gaussian (log_std, log-probs); with OU noise and the clamp (ActorOuW); the
// five-output head under a Categorical (ActorCatW); the last two storing 16-bit observations (obs_fmt); and the five-output head
// under Gumbel noise (ActorGumW).
enum ActorMember { ACTOR_DET, ACTOR_GAUSS, ACTOR_OU, ACTOR_CAT, ACTOR_GAUSS16, ACTOR_CAT16, ACTOR_GUMBEL };
__host__ __device__ constexpr bool actor_member_sample(ActorMember m) { return m == ACTOR_GAUSS || m == ACTOR_GAUSS16; }
__host__ __device__ constexpr bool actor_member_ou(ActorMember m) { return m == ACTOR_OU; }
__host__ __device__ constexpr bool actor_member_cat(ActorMember m) { return m == ACTOR_CAT || m == ACTOR_CAT16; }
__host__ __device__ constexpr bool actor_member_obs16(ActorMember m) { return m == ACTOR_GAUSS16 || m == ACTOR_CAT16; }
__host__ __device__ constexpr bool actor_member_gumbel(ActorMember m) { return m == ACTOR_GUMBEL; }
__host__ __device__ constexpr bool actor_member_head5(ActorMember m) { return actor_member_cat(m) || actor_member_gumbel(m); }   // a head of five
__host__ __device__ constexpr bool actor_obs16_shape(int n, int h) { return (n == 3 || n == 9 || n == 27) && (h == 32 || h == 64); }  // built for

// floats of b1 | b2 | W3 in LDS (a per-agent family reads them through L1), and of the b3 | log_std slot behind them
// (head5: a head of five, actor_member_head5)
__host__ __device__ constexpr int actor_w_floats(int h, bool per_agent, bool head5) { return per_agent ? 0 : (head5 ? 2 + FG_CAT : 4) * h; }
__host__ __device__ constexpr int actor_b3_floats(bool head5) { return head5 ? 8 : 4; }
// The LDS of one workgroup: the float offset of every block behind the env blocks [E][env_block_floats], and the total.  A
// block a kernel does not have is empty; the body takes its pointers, and the host the launch's bytes, from this one function.
// (E N is a multiple of 8, so the [E N] blocks keep every later block 32-byte aligned.)
struct ActorLds {
    int act;      // actions [E N][2]
    int logp;     // Gaussian and categorical members: log-probs [E N]
    int idx;      // a head of five (categorical and Gumbel members): indices [E N]
    int wsm;      // b1 [H] b2 [H] W3 [2][H] (not per_agent) | b3 [2], then log_std [2] (Gaussian members) or padding;
                  // a head of five: b1 [H] b2 [H] W3 [5][H] | b3 [5] and padding to 8
    int ln;       // lnorm: gamma1 [H] beta1 [H] gamma2 [H] beta2 [H] gamma0 [DP] beta0 [DP], DP = 6N rounded up to 4
    int bn;       // in_bn, not per_agent: mean [DP] istd [DP] gamma [DP] beta [DP] of the input BatchNorm
    int gru;      // gru: b_ir + b_hr [H] b_iz + b_hz [H] b_in [H] b_hn [H] gamma3 [H] beta3 [H]
    int tiles;    // activations [4][32][H + 4]
    int state;    // gru: hidden state [TILES 32][H + 4], TILES = ceil(E N / 32); the OU member: noise state [E N][2]
    int total;
};
__host__ __device__ constexpr ActorLds actor_lds_layout(int n, int h, ActorFlags f, ActorMember m) {
    const bool cat = actor_member_cat(m), head5 = actor_member_head5(m);
    const int rows = actor_envs(n) * n, dp = actor_in_pad(n), hs = actor_hstride(h);
    ActorLds l{};
    l.act = actor_envs(n) * env_block_floats(n);
    l.logp = l.act + 2 * rows;
    l.idx = l.logp + (actor_member_sample(m) || cat ? rows : 0);
    l.wsm = l.idx + (head5 ? rows : 0);
    l.ln = l.wsm + actor_w_floats(h, f.per_agent, head5) + actor_b3_floats(head5);
    l.bn = l.ln + (f.lnorm ? 4 * h + 2 * dp : 0);
    l.gru = l.bn + (f.in_bn && !f.per_agent ? 4 * dp : 0);
    l.tiles = l.gru + (f.gru ? 6 * h : 0);
    l.state = l.tiles + (FG_ACTOR_THREADS / 64) * FG_ACTOR_ROWS * hs;
    l.total = l.state + (f.gru ? actor_state_rows(n) * hs : 0) + (actor_member_ou(m) ? 2 * rows : 0);
    return l;
}
__host__ __device__ constexpr int actor_lds_floats(int n, int h, ActorFlags f, ActorMember m) { return actor_lds_layout(n, h, f, m).total; }
__host__ __device__ constexpr int actor_lds_bytes(int n, int h, ActorFlags f, ActorMember m) { return 4 * actor_lds_floats(n, h, f, m); }

// The exploration noise eps [2] of agent i of global env g for the step whose counter offset is `offset`: its own Philox
// stream, word 1 = i ^ 0xA0000000 (motor_noise flips bit 31 of i | 0x20000000).  The other streams keyed by (g, i, offset):
// auto-reset {g, i} and {g, 0xFFFFFFFF}, motor noise i ^ 0x80000000, communication noise (i | 0x40000000 | q << 12) ^ 0x80000000
// - top three bits 000 / 111, 100, 110 against 101 here, for every i < 2^29.
FG_DEV float2 actor_eps(uint64_t seed, uint32_t g, uint32_t i, uint64_t offset) {
    const real2 n = motor_noise(seed, g, i | 0x20000000u, offset);
    return make_float2((float)n.x, (float)n.y);
}

// The log-density of the standard-normal pair n under N(mean, diag(exp(log_std))^2) at mean + exp(log_std) n:
// -0.5 |n|^2 - (ls0 + ls1) - log(2 pi).  The one spelling for the shared, per-agent and landmark kernels.
FG_DEV float gauss_logp(float2 n, float ls0, float ls1) {
    return -0.5f * (n.x * n.x + n.y * n.y) - (ls0 + ls1) - 1.8378770664093453f;
}

// The uniform draw u in [0, 1) of agent i of global env g for the step whose counter offset is `offset` (the categorical
// members): word 2 of actor_eps's Philox block - key `seed`, counter {g, i ^ 0xA0000000, lo32(offset), hi32(offset)} - as
// (c[2] >> 8) 2^-24.  Words 0 and 1 stay the Gaussian members' draw.
FG_DEV float actor_uniform(uint64_t seed, uint32_t g, uint32_t i, uint64_t offset) {
    uint32_t c[4] = {g, i ^ 0xA0000000u, (uint32_t)offset, (uint32_t)(offset >> 32)};
    philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (float)(c[2] >> 8) * (1.0f / 16777216.0f);
}

// The Categorical over five fp32 logits, the one spelling for the fused kernels and fg_actor_categorical, in fp32:
//     m = max_j l_j,   e_j = exp(l_j - m),   c_j = e_0 + .. + e_j (ascending),   s = c_4
//     sampled: t = u s, idx the first j in 0..3 with t < c_j, else 4;   greedy: idx the lowest index attaining m
//     log_prob = (l_idx - m) - log(s)
// exp and log are __expf and __logf (v_exp_f32 / v_log_f32 behind one multiply): about 2 ulp on e_j in (0, 1] and on log(s),
// s in [1, 5]; a class further than ~87 below the maximum underflows to e_j = 0 and is never sampled.
struct CatPick { int idx; float logp; };
FG_DEV CatPick cat_pick(const float (&l)[FG_CAT], float u, bool greedy) {
    float m = l[0];
#pragma unroll
    for (int j = 1; j < FG_CAT; ++j) m = fmaxf(m, l[j]);
    float c[FG_CAT];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < FG_CAT; ++j) { s += __expf(l[j] - m); c[j] = s; }
    const float t = u * s;
    int idx = FG_CAT - 1;
    float li = l[FG_CAT - 1];
#pragma unroll
    for (int j = FG_CAT - 2; j >= 0; --j) {            // descending, so that the lowest index that qualifies stays
        const bool take = greedy ? l[j] == m : t < c[j];
        idx = take ? j : idx;
        li = take ? l[j] : li;
    }
    return {idx, (li - m) - __logf(s)};
}
// The index as the env's raw action u (MultiAgentEnv._set_action): FG_ACT_ONEHOT5 takes the one-hot e_idx through
// u = (a1 - a2, a3 - a4) - 1: +x, 2: -x, 3: +y, 4: -y - and FG_ACT_INDEX is decode_actions_kernel's 1: -x, 2: +x, 3: -y, 4: +y;
// index 0 is no move in both.
FG_DEV float2 cat_decode(int mode, int idx) {
    const float sgn = mode == FG_ACT_INDEX ? -1.0f : 1.0f;
    return make_float2(idx == 1 ? sgn : idx == 2 ? -sgn : 0.0f, idx == 3 ? sgn : idx == 4 ? -sgn : 0.0f);
}

// The five Gumbel draws g [5] of agent i of global env g for the step whose counter offset is `offset` (the Gumbel members): a
// Philox stream of its own - key `seed`, counter {g, i | 0x60000000 | q << 12, lo32(offset), hi32(offset)}, draw j from word j & 3
// of block q = j >> 2 - whose word 1 has the top three bits 011 for every i < 2^12, against 000 / 001 / 100 / 101 / 110 / 111 of
// the other streams (actor_eps above), so that no other draw moves.  u_j = (2 (c >> 9) + 1) 2^-24 is an odd 24-bit integer
// scaled: exact in fp32 and strictly inside (0, 1), so neither logarithm sees 0 or 1; g_j = -log(-log(u_j)) in [-2.82, 16.64].
// Both logarithms are the math library's full-precision one (about 1 ulp) and NOT logf / __logf, which this build's
// -fapprox-func lowers to v_log_f32 and one multiply: the inner result is the outer logarithm's argument, and next to u = 1
// the hardware instruction's absolute error is not small against -ln u.
extern "C" __device__ float __ocml_log_f32(float);
FG_DEV float gumbel_log(float x) { return __ocml_log_f32(x); }
FG_DEV void actor_gumbel(uint64_t seed, uint32_t g, uint32_t i, uint64_t offset, float (&out)[FG_CAT]) {
#pragma unroll
    for (uint32_t q = 0; q < (FG_CAT + 3) / 4; ++q) {
        uint32_t c[4] = {g, i | 0x60000000u | (q << 12), (uint32_t)offset, (uint32_t)(offset >> 32)};
        philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
        for (int wd = 0; wd < 4; ++wd) {
            const int j = (int)q * 4 + wd;
            if (j < FG_CAT) {
                const float u = (float)(2u * (c[wd] >> 9) + 1u) * (1.0f / 16777216.0f);
                out[j] = -gumbel_log(-gumbel_log(u));
            }
        }
    }
}
// MADDPG's discrete action from five fp32 logits, the one spelling for the fused kernels and fg_actor_gumbel_pick: exploring
// (gumbel_softmax(logits, hard=True)), y_j = l_j + g_j - one fp32 addition of the finished logit, never contracted into its
// chain - else (onehot_from_logits) y_j = l_j and g is not read; the index is the lowest j attaining max_j y_j.  The
// temperature does not enter: argmax softmax(y / T) = argmax y for every T > 0.
FG_DEV int gumbel_pick(const float (&l)[FG_CAT], const float (&g)[FG_CAT], bool explore) {
#pragma clang fp contract(off)
    float y[FG_CAT];
#pragma unroll
    for (int j = 0; j < FG_CAT; ++j) y[j] = explore ? l[j] + g[j] : l[j];
    float m = y[0];
#pragma unroll
    for (int j = 1; j < FG_CAT; ++j) m = fmaxf(m, y[j]);
    int idx = FG_CAT - 1;
#pragma unroll
    for (int j = FG_CAT - 2; j >= 0; --j) idx = y[j] == m ? j : idx;   // descending, so that the lowest index that qualifies stays
    return idx;
}

// The pieces of one wave pass of the actor MLP (fg_actor_mlp.inc) that layer 1 of each body shares with it.  acc: the pass's
// accumulators, register j of lane l holding row 4 (l >> 4) + j, column l & 15 of its 16 x 16 tile; col = l & 15, kq = l >> 4.
// The bias (H floats in LDS) as the accumulators' initial value:
template <int RT, int CB>
FG_DEV void actor_bias_init(f32x4 (&acc)[RT][CB], const float* bias, int col) {
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) {
        const float bv = bias[cb * 16 + col];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][cb] = (f32x4){bv, bv, bv, bv};
    }
}
// ReLU -> the wave's activation tile hb [16 RT][HS]:
template <int RT, int CB>
FG_DEV void actor_store_tile(float* hb, int HS, const f32x4 (&acc)[RT][CB], int col, int kq) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int cb = 0; cb < CB; ++cb)
#pragma unroll
            for (int j = 0; j < 4; ++j) hb[(rt * 16 + kq * 4 + j) * HS + cb * 16 + col] = fmaxf(acc[rt][cb][j], 0.f);
}

// LayerNorm over each row of the wave's activation tile hb [FG_ACTOR_ROWS][HS], in place (LNORM kernels): gb = gamma [H] |
// beta [H] in LDS.  Lane = (row lane >> 2 of 16, c = lane & 3) holds columns c, c + 4, ... of its row in registers: the mean,
// then the centred sum of squares, each finished by two DPP quad steps (the four lanes of a row end with the same bits).
// A row of zeros comes back as beta exactly.  The caller orders it against the tile's writers and readers (WaveSync).
template <int H>
FG_DEV void actor_row_norm(float* hb, int HS, const float* gb, float eps, int lane) {
    const int c = lane & 3;
#pragma unroll
    for (int part = 0; part < FG_ACTOR_ROWS / 16; ++part) {
        float* const hr = hb + (part * 16 + (lane >> 2)) * HS + c;
        float x[H / 4];
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < H / 4; ++j) { x[j] = hr[4 * j]; sum += x[j]; }
        sum = bfly<2, R_SUM>(bfly<1, R_SUM>(sum));
        const float mean = sum * (1.0f / (float)H);
        float ssq = 0.f;
#pragma unroll
        for (int j = 0; j < H / 4; ++j) { x[j] -= mean; ssq = __builtin_fmaf(x[j], x[j], ssq); }
        ssq = bfly<2, R_SUM>(bfly<1, R_SUM>(ssq));
        const float rstd = 1.0f / sqrtf(ssq * (1.0f / (float)H) + eps);
#pragma unroll
        for (int j = 0; j < H / 4; ++j) hr[4 * j] = __builtin_fmaf(x[j] * rstd, gb[4 * j + c], gb[H + 4 * j + c]);
    }
}

// One step's eps for every (env, agent) at rng_base(p) (fg_actor_noise): the host-paced loop of a Gaussian actor draws
// what actor_sample_kernel draws.
__global__ __launch_bounds__(256) void actor_noise_kernel(const KParams p, int B, int N, float2* __restrict__ eps) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)B * N) return;
    const int b = (int)(t / N), i = (int)(t - (long long)b * N);
    eps[t] = actor_eps(p.seed, (uint32_t)(b + p.env_index_base), (uint32_t)i, rng_base(p));
}

// The log-density of each of `count` draws eps [count][2] under log_std [2] (fg_actor_log_prob): gauss_logp on the values the
// fused kernels give it, so that the host-paced loop of a Gaussian actor returns the fused launch's bits.
__global__ __launch_bounds__(256) void actor_logp_kernel(long long count, const float2* __restrict__ eps,
                                                         const float* __restrict__ log_std, float* __restrict__ logp) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    logp[t] = gauss_logp(eps[t], log_std[0], log_std[1]);
}

// One step's uniform draw for every (env, agent) at rng_base(p) (fg_actor_uniform): the host-paced loop of a CategoricalActor
// draws what the *cat_actor_kernel draw.
__global__ __launch_bounds__(256) void actor_uniform_kernel(const KParams p, int B, int N, float* __restrict__ u) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)B * N) return;
    const int b = (int)(t / N), i = (int)(t - (long long)b * N);
    u[t] = actor_uniform(p.seed, (uint32_t)(b + p.env_index_base), (uint32_t)i, rng_base(p));
}

// cat_pick and cat_decode on each of `count` rows of caller-supplied logits [count][5] and draws u [count]
// (fg_actor_categorical): the host-paced loop of a CategoricalActor takes the fused launch's arithmetic from its own logits.
__global__ __launch_bounds__(256) void actor_categorical_kernel(int mode, int greedy, long long count,
                                                                const float* __restrict__ logits, const float* __restrict__ u,
                                                                int* __restrict__ idx, float2* __restrict__ act,
                                                                float* __restrict__ logp) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    float l[FG_CAT];
#pragma unroll
    for (int j = 0; j < FG_CAT; ++j) l[j] = logits[t * FG_CAT + j];
    const CatPick pk = cat_pick(l, greedy ? 0.f : u[t], greedy != 0);
    idx[t] = pk.idx;
    if (act) act[t] = cat_decode(mode, pk.idx);
    if (logp) logp[t] = pk.logp;
}

// One step's five Gumbel draws for every (env, agent) at rng_base(p) (fg_actor_gumbel): the host-paced loop of a
// GumbelSoftmaxActor draws what the *gumbel_actor_kernel draw.
__global__ __launch_bounds__(256) void actor_gumbel_kernel(const KParams p, int B, int N, float* __restrict__ g) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)B * N) return;
    const int b = (int)(t / N), i = (int)(t - (long long)b * N);
    float d[FG_CAT];
    actor_gumbel(p.seed, (uint32_t)(b + p.env_index_base), (uint32_t)i, rng_base(p), d);
#pragma unroll
    for (int j = 0; j < FG_CAT; ++j) g[t * FG_CAT + j] = d[j];
}

// gumbel_pick and cat_decode on each of `count` rows of caller-supplied logits [count][5] and draws g [count][5] (NULL when not
// exploring) (fg_actor_gumbel_pick): the host-paced loop of a GumbelSoftmaxActor takes the fused launch's arithmetic from its
// own logits.
__global__ __launch_bounds__(256) void actor_gumbel_pick_kernel(int mode, int explore, long long count,
                                                                const float* __restrict__ logits, const float* __restrict__ g,
                                                                int* __restrict__ idx, float2* __restrict__ act) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    float l[FG_CAT], d[FG_CAT];
#pragma unroll
    for (int j = 0; j < FG_CAT; ++j) {
        l[j] = logits[t * FG_CAT + j];
        d[j] = explore ? g[t * FG_CAT + j] : 0.f;
    }
    const int pk = gumbel_pick(l, d, explore != 0);
    idx[t] = pk;
    if (act) act[t] = cat_decode(mode, pk);
}

// ou_step on each of `count` (env, agent) pairs in place (fg_actor_ou_step): the host-paced loop of an OUNoiseActor carries
// the state the fused kernels carry, from the same eps.
__global__ __launch_bounds__(256) void actor_ou_step_kernel(long long count, float theta, float mu, float sigma,
                                                            const float2* __restrict__ eps, float2* __restrict__ state) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    const float2 x = state[t], n = eps[t];
    state[t] = make_float2(ou_step(x.x, n.x, theta, mu, sigma), ou_step(x.y, n.y, theta, mu, sigma));
}

// ---- the kernels: one block per family around fg_actor_family.inc.  The body names all of `w tab nw gw bw btab ow cw gum`, and an
// operand a kernel does not take is the empty constant below (`w` of a per-agent family: only tab's tanh flag), so that no
// kernel carries an argument it never reads.
#define FG_ACTOR_NO_W     const ActorW w = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, tab.out_tanh};
#define FG_ACTOR_NO_TAB   constexpr ActorTab tab{};
#define FG_ACTOR_NO_NW    constexpr ActorNormW nw{};
#define FG_ACTOR_NO_GW    constexpr ActorGruW gw{};
#define FG_ACTOR_NO_BW    constexpr ActorBnW bw{};
#define FG_ACTOR_NO_BTAB  constexpr ActorBnTab btab{};
#define FG_ACTOR_NO_OW    constexpr ActorOuW ow{};
#define FG_ACTOR_NO_CW    constexpr ActorCatW cw{};
#define FG_ACTOR_NO_GUM   constexpr ActorGumW gum{};
#define FG_ACTOR_NO_GAUSS const float* const log_std = nullptr; float* const logp = nullptr;
#define FG_ACTOR_NO_OBS16 constexpr int obs_fmt = 0;
// what the body reads of its kernel: the member and the family's flags, each fact from the one predicate or field
#define FG_ACTOR_IS(M)                                                                                                         \
    constexpr ActorMember MEMBER = M;                                                                                          \
    constexpr ActorFlags FLAGS = FG_ACTOR_FLAGS;                                                                               \
    constexpr bool SAMPLE = actor_member_sample(M), OU = actor_member_ou(M), CAT = actor_member_cat(M), OBS16 = actor_member_obs16(M), \
                   GUM = actor_member_gumbel(M),                                                                               \
                   PER_AGENT = FLAGS.per_agent, LNORM = FLAGS.lnorm, GRU = FLAGS.gru, INBN = FLAGS.in_bn;                      \
    FG_ACTOR_ABSENT
#define FG_ACTOR_STR_(x) #x
#define FG_ACTOR_STR(x) FG_ACTOR_STR_(x)

// One kind per entry point fg_rollout_hd_actor* (formation_hip.hip: hd_actor_entry); HD_ACTOR_SAMPLE shares the shared family's kernels.
enum HdActorKind { HD_ACTOR_SHARED, HD_ACTOR_SAMPLE, HD_ACTOR_PER_AGENT, HD_ACTOR_NORM, HD_ACTOR_GRU, HD_ACTOR_BN,
                   HD_ACTOR_BN_PER_AGENT };
template <HdActorKind> struct HdActorFamily;

// the shared actor
#define FG_ACTOR_KIND     HD_ACTOR_SHARED
#define FG_ACTOR_MAXH     128
#define FG_ACTOR_WHAT     ""
#define FG_ACTOR_FLAGS    ActorFlags{/* per_agent */ false, /* lnorm */ false, /* gru */ false, /* in_bn */ false}
#define FG_ACTOR_OPERANDS const ActorW w
#define FG_ACTOR_ABSENT   FG_ACTOR_NO_BW FG_ACTOR_NO_BTAB FG_ACTOR_NO_NW FG_ACTOR_NO_GW FG_ACTOR_NO_TAB
#define FG_ACTOR_DET      actor_rollout_kernel
#define FG_ACTOR_SMP      actor_sample_kernel
#define FG_ACTOR_OUK      ou_actor_kernel
#define FG_ACTOR_GUMK     gumbel_actor_kernel
#define FG_ACTOR_CATK     cat_actor_kernel
#define FG_ACTOR_SMP16    actor_sample_obs16
#define FG_ACTOR_CAT16    cat_actor_obs16
#include "fg_actor_family.inc"
template <> struct HdActorFamily<HD_ACTOR_SAMPLE> : HdActorFamily<HD_ACTOR_SHARED> {};

// per_agent: agent i evaluates tab's actor i; the Gaussian member has one log_std [2] for all agents
#define FG_ACTOR_KIND     HD_ACTOR_PER_AGENT
#define FG_ACTOR_MAXH     128
#define FG_ACTOR_WHAT     "per-agent "
#define FG_ACTOR_FLAGS    ActorFlags{/* per_agent */ true, /* lnorm */ false, /* gru */ false, /* in_bn */ false}
#define FG_ACTOR_OPERANDS const ActorTab tab
#define FG_ACTOR_ABSENT   FG_ACTOR_NO_BW FG_ACTOR_NO_BTAB FG_ACTOR_NO_NW FG_ACTOR_NO_GW FG_ACTOR_NO_W
#define FG_ACTOR_DET      pa_actor_kernel
#define FG_ACTOR_SMP      pa_sample_kernel
#define FG_ACTOR_OUK      pa_ou_actor_kernel
#define FG_ACTOR_GUMK     pa_gumbel_actor_kernel
#include "fg_actor_family.inc"

// lnorm: the shared actor with LayerNorms `nw`
#define FG_ACTOR_KIND     HD_ACTOR_NORM
#define FG_ACTOR_MAXH     64
#define FG_ACTOR_WHAT     "LayerNorm "
#define FG_ACTOR_FLAGS    ActorFlags{/* per_agent */ false, /* lnorm */ true, /* gru */ false, /* in_bn */ false}
#define FG_ACTOR_OPERANDS const ActorW w, const ActorNormW nw
#define FG_ACTOR_ABSENT   FG_ACTOR_NO_BW FG_ACTOR_NO_BTAB FG_ACTOR_NO_GW FG_ACTOR_NO_TAB
#define FG_ACTOR_DET      ln_actor_kernel
#define FG_ACTOR_SMP      ln_sample_kernel
#define FG_ACTOR_CATK     ln_cat_actor_kernel
#define FG_ACTOR_SMP16    ln_sample_obs16
#define FG_ACTOR_CAT16    ln_cat_actor_obs16
#include "fg_actor_family.inc"

// gru: the LayerNorm actor with the recurrent layer `gw` before its head
#define FG_ACTOR_KIND     HD_ACTOR_GRU
#define FG_ACTOR_MAXH     64
#define FG_ACTOR_WHAT     "recurrent "
#define FG_ACTOR_FLAGS    ActorFlags{/* per_agent */ false, /* lnorm */ true, /* gru */ true, /* in_bn */ false}
#define FG_ACTOR_OPERANDS const ActorW w, const ActorNormW nw, const ActorGruW gw
#define FG_ACTOR_ABSENT   FG_ACTOR_NO_BW FG_ACTOR_NO_BTAB FG_ACTOR_NO_TAB
#define FG_ACTOR_DET      gru_actor_kernel
#define FG_ACTOR_SMP      gru_sample_kernel
#define FG_ACTOR_CATK     gru_cat_actor_kernel
#define FG_ACTOR_SMP16    gru_sample_obs16
#define FG_ACTOR_CAT16    gru_cat_actor_obs16
#include "fg_actor_family.inc"

// in_bn: the shared actor behind the eval-mode input BatchNorm `bw`
#define FG_ACTOR_KIND     HD_ACTOR_BN
#define FG_ACTOR_MAXH     64
#define FG_ACTOR_WHAT     "BatchNorm "
#define FG_ACTOR_FLAGS    ActorFlags{/* per_agent */ false, /* lnorm */ false, /* gru */ false, /* in_bn */ true}
#define FG_ACTOR_OPERANDS const ActorW w, const ActorBnW bw
#define FG_ACTOR_ABSENT   FG_ACTOR_NO_NW FG_ACTOR_NO_GW FG_ACTOR_NO_TAB FG_ACTOR_NO_BTAB
#define FG_ACTOR_DET      bn_actor_kernel
#define FG_ACTOR_SMP      bn_sample_kernel
#define FG_ACTOR_OUK      bn_ou_actor_kernel
#define FG_ACTOR_GUMK     bn_gumbel_actor_kernel
#include "fg_actor_family.inc"

// in_bn, per_agent: agent i evaluates tab's actor i behind btab's BatchNorm i
static_assert(sizeof(Args) + sizeof(ActorTab) + sizeof(ActorBnTab) + 2 * sizeof(void*) <= 4096, "kernel arguments: 4 KiB");
static_assert(sizeof(Args) + sizeof(ActorTab) + sizeof(ActorBnTab) + sizeof(ActorOuW) <= 4096, "kernel arguments: 4 KiB");
#define FG_ACTOR_KIND     HD_ACTOR_BN_PER_AGENT
#define FG_ACTOR_MAXH     64
#define FG_ACTOR_WHAT     "per-agent BatchNorm "
#define FG_ACTOR_FLAGS    ActorFlags{/* per_agent */ true, /* lnorm */ false, /* gru */ false, /* in_bn */ true}
#define FG_ACTOR_OPERANDS const ActorTab tab, const ActorBnTab btab
#define FG_ACTOR_ABSENT   FG_ACTOR_NO_NW FG_ACTOR_NO_GW FG_ACTOR_NO_BW FG_ACTOR_NO_W
#define FG_ACTOR_DET      pa_bn_actor_kernel
#define FG_ACTOR_SMP      pa_bn_sample_kernel
#define FG_ACTOR_OUK      pa_bn_ou_actor_kernel
#define FG_ACTOR_GUMK     pa_bn_gumbel_actor_kernel
#include "fg_actor_family.inc"

#undef FG_ACTOR_NO_W
#undef FG_ACTOR_NO_TAB
#undef FG_ACTOR_NO_NW
#undef FG_ACTOR_NO_GW
#undef FG_ACTOR_NO_BW
#undef FG_ACTOR_NO_BTAB
#undef FG_ACTOR_NO_OW
#undef FG_ACTOR_NO_CW
#undef FG_ACTOR_NO_GUM
#undef FG_ACTOR_NO_GAUSS
#undef FG_ACTOR_NO_OBS16
#undef FG_ACTOR_IS
#undef FG_ACTOR_STR_
#undef FG_ACTOR_STR

}  // namespace fg

#endif  // FG_ACTOR_ROLLOUT_KERNEL_HPP_
