// fg_returns_kernel.hpp - Discounted returns of C candidate action sequences from the CURRENT state (fg_rollout_hd_returns).
// Part of libformation_hip (gfx950); included by formation_hip.hip, one translation unit - and, with real = double, by the
// tests' parity build formation_hip_f64.hip (fg64_rollout_hd_returns: the same geometry per agent count).
#ifndef FG_RETURNS_KERNEL_HPP_
#define FG_RETURNS_KERNEL_HPP_

#include "fg_common.hpp"
#include "fg_pair_loops.hpp"

namespace fg {

// ---------------------------------------------------------------------------
// K steps of World.step + reward for every (candidate c, env b) pair, each from env b's current state, reduced on the chip
// to two discounted sums per agent.  The state is read and never written: a planner (random shooting, CEM, MPPI) scores its
// candidates and the env stays where it was.
//   one lane group of G lanes per pair, agents on lanes as in step_kernel and the rollout producers (the G those kernels
//   use for the same N); T / G pairs per workgroup; pair q = b C + c, so that the candidates of one env are neighbours (one
//   workgroup, or consecutive ones) and their state loads hit in L2.
// Everything a pair needs from other lanes comes from its own wave (G <= 64): LDS operations of one wave complete in order and
// the reductions are in-register butterflies, so there is no workgroup barrier, no table, no writer wave and no atomic.  The
// launch stores 8 N + 4 bytes per pair and reads 8 N bytes per pair and step: it is bound by the step's dependent chain
// (pair loops, transcendentals, butterflies), which more resident waves hide - hence small LDS (6 NP floats per pair: never
// the limit) and the occupancy attribute of returns_kernel.
// LDS per pair (floats): QX QY PX PY SX SY [NP] - the pair loops' arrays of rollout_kernel's env block, without its tables.
// ---------------------------------------------------------------------------
__host__ __device__ constexpr int returns_block_floats(int n) { return 6 * npad(n); }
template <int NC, int G, int T> constexpr int returns_lds_bytes() { return (T / G) * returns_block_floats(NC) * (int)sizeof(real); }

struct ReturnsArgs {
    KParams p;                 // auto_reset is ignored: no reset is drawn, the RNG is not touched
    int B, K, C;
    real gamma;
    const real* px; const real* py; const real* vx; const real* vy;   // [B][N]
    const real* shape;         // [B][N][2]
    const real* ivel;          // [B][2]
    const int32_t* step;       // [B]
    const real* act;           // [C][K][B][N][2]
    real* ret;                 // [C][B][N]  sum of gamma^k shared_k over the counted steps
    real* indiv_ret;           // [C][B][N]  ... of own_k, or NULL
    int32_t* steps;            // [B] counted steps, or NULL
};

// One geometry per agent count: T = 256 threads (one wave per SIMD and workgroup; 64 / 32 / 16 / 8 pairs at G = 4 / 8 / 16 / 32),
// no workgroup barrier, so the workgroup size only sets the dispatch grain - 4096 pairs of 27 agents are 512 workgroups, two
// per CU - and the occupancy comes from the registers.  waves_per_eu(4) is the 128-register budget the producers' step was
// written for (rollout_kernel's small workgroups): the compiler then takes 66 ... 100 (3 / 4 agents 68 / 66, 8: 82, 9: 100,
// 16: 88, 25 / 27 / 32: 80), which is 7 ... 4 resident waves per SIMD to cover one wave's chain.  Asking for more costs
// scratch: a minimum of 6 spills 18 registers at 9 agents and 8 at 16, a budget of 64 (8 waves) 14 ... 28 in every instantiation.
// The budget was sized for floats: the fp64 parity build (tests only) spills 45 ... 142 registers under it, so the attribute is
// the product's alone and the doubles get what __launch_bounds__ allows.
#if FG_F64
#define FG_RETURNS_OCCUPANCY
#else
#define FG_RETURNS_OCCUPANCY __attribute__((amdgpu_waves_per_eu(4)))
#endif
template <int NC, int G, int T>
__global__ __launch_bounds__(T) FG_RETURNS_OCCUPANCY
void returns_kernel(const ReturnsArgs a) {
#define FG_RETURNS_SAMPLED 0
#include "fg_returns_body.inc"
#undef FG_RETURNS_SAMPLED
}

}  // namespace fg

#endif  // FG_RETURNS_KERNEL_HPP_
