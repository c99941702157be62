// formation_hip_f64.hip - "parity mode" build of the fused step kernel: the SAME kernel source as
// libformation_hip (fg_step_kernel.hpp, fg_pair_loops.hpp, the reductions of fg_common.hpp) compiled with
// real = double, run-time agent count, flat observation writer - and of the pipelined rollout kernel
// (fg_rollout_kernels.hpp: rollout_kernel<9 | 27, ...> and rollout_kernel_wide<81 | 243, ...> with the rows writer).  TEST INFRASTRUCTURE ONLY (tests/test_gpu_f64_parity.py):
// it lets the kernel's algorithm free-run against the reference's float64 trajectories
// (/root/reference/formation_gym/core.py:206-225, :289-322; environment.py:113-142) over whole fixtures, which an
// fp32 run cannot do beyond ~10 steps because stiff contacts amplify rounding chaotically.  Not shipped in the
// product path: formation_gym never loads it.
// Both halves of step_kernel are built: OPTS = false (fg64_step_hd) and OPTS = true (fg64_step_hd_opts: accel, max_speed, walls
// with corner rounding / soft walls / ghosts, the per-agent table with its mass ratio, per-pair contact and penalty distances,
// immovable / non-colliding / scripted agents, the communication block of the flat writer, the 1024-thread re-fetch of the
// properties, the K-loop), each free-running on the reference's option fixtures (tests/test_gpu_f64_options.py).
// fg64_rollout_scenario is the run-time-count kernel of the four landmark scenarios (fg_scn_kernel.hpp: scn_kernel<G, T> at every
// lane-group width 4 ... 64 and every whole-workgroup size 128 ... 1024, both observation writers, the K-loop, per-agent tables and
// walls), free-running on the 14 landmark fixtures (tests/test_gpu_f64_scenarios.py).
// fg64_rollout_hd_returns is returns_kernel<N, G, 256> (fg_returns_kernel.hpp) at the product's lane group per agent count: the
// discounted returns of candidate action sequences against float64 sums over the reference's steps (tests/test_gpu_f64_returns.py).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=on -DFG_F64=1 -fPIC -shared -Iinclude
//         -o lib/libformation_hip_f64.so csrc/formation_hip_f64.hip          (no -fapprox-func: full-precision libm)
#define FG_F64 1
#include "fg_common.hpp"
#include "fg_pair_loops.hpp"
#include "fg_step_kernel.hpp"
#include "fg_rollout_kernels.hpp"
#include "fg_scn_kernel.hpp"
#include "fg_returns_kernel.hpp"

namespace fg {

// returns_kernel<N, G, 256> with real = double at the product's geometry (returns_dispatch, formation_hip.hip): the pair-per-wave
// layout under test is the one that ships.  LDS is (256 / G) pairs x 6 NP doubles: 12 KB at most, inside the default limit.
template <int NC, int G>
static int launch_returns64(const ReturnsArgs& a, hipStream_t st) {
    constexpr int T = 256, PW = T / G;
    constexpr int lds = returns_lds_bytes<NC, G, T>();
    static_assert(lds <= 64 * 1024, "the parity build stays inside the default LDS limit");
    const unsigned grid = (unsigned)(((long long)a.B * a.C + PW - 1) / PW);
    hipLaunchKernelGGL((returns_kernel<NC, G, T>), dim3(grid), dim3(T), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// The pipelined producer / writer rollout kernel (fg_rollout_kernels.hpp) with real = double: the SAME source as the product's
// rollout_kernel<N, G, TP, TW, E, 0, 0, false> - producer waves, double-buffered LDS tables, the rows writer - so that the K-step
// path has its own whole-fixture free-running check against the reference's fp64 trajectories.
template <int NC, int G, int TP, int TW, int E>
static hipError_t launch_roll64(const Args& a, hipStream_t st) {
    const int grid = (a.B + E - 1) / E;
    constexpr int lds = roll_lds_bytes<NC, TW, E, 0, 0>();
    static_assert(lds <= 64 * 1024, "the parity build stays inside the default LDS limit");
    hipLaunchKernelGGL((rollout_kernel<NC, G, TP, TW, E, 0, 0, false>), dim3(grid), dim3(TP + TW), lds, st, a);
    return hipGetLastError();
}

// ... and the one-env-per-producer-wave form for 81 / 243 agents (rollout_kernel_wide)
template <int NC, int A, int E, int TW>
static hipError_t launch_wide64(Args a, hipStream_t st) {
    a.groups = 1;
    const int grid = (a.B + E - 1) / E;
    constexpr int lds = E * roll_block_floats(NC) * (int)sizeof(real);
    static_assert(lds <= 64 * 1024, "the parity build stays inside the default LDS limit");
    hipLaunchKernelGGL((rollout_kernel_wide<NC, A, E, TW, 0, false>), dim3(grid), dim3(E * 64 + TW), lds, st, a);
    return hipGetLastError();
}

constexpr int FG64_LDS_LIMIT = 160 * 1024;      // LDS one gfx950 workgroup can have

// -2: the workgroup's LDS does not fit (OPTS from ~970 agents up: 8-byte tables); -4: the runtime refused; 0: launched
template <int G, int T, int E, bool IDX, bool OPTS>
static int launch64(const Args& a, hipStream_t st) {
    const int grid = (a.B + E - 1) / E;
    const int lds = step_lds_bytes(a.N, E, OPTS);           // the product host side's arithmetic (fg_common.hpp), sizeof(real) = 8
    if (lds > FG64_LDS_LIMIT) return -2;
    const auto kernel = &step_kernel<0, G, T, E, IDX, OPTS>;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return -4;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(T), lds, st,
                       a.B, a.N, (const real*)a.px, (const real*)a.py, (const real*)a.vx, (const real*)a.vy,
                       (const real*)a.shape, (const real*)a.ivel, (const int32_t*)a.step, a);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// The geometry table of the run-time-N step kernel: lanes per env, threads and envs per workgroup by agent count
// (the product's NC = 0 variants, formation_hip.hip kVariants).  OPTS always carries the index outputs, as in the product.
static int launch_step64(const Args& a, bool idx, bool opts, hipStream_t st) {
    int G = 4; while (G < a.N) G <<= 1;
    if (G > 64 && G < 128) G = 128;
#define FG64(GG, TT, EE) return opts ? launch64<GG, TT, EE, true, true>(a, st) \
                              : idx ? launch64<GG, TT, EE, true, false>(a, st) : launch64<GG, TT, EE, false, false>(a, st)
    switch (G) {
        case 4: FG64(4, 64, 16);      case 8: FG64(8, 64, 8);       case 16: FG64(16, 64, 4);
        case 32: FG64(32, 128, 4);    case 64: FG64(64, 128, 2);    case 128: FG64(128, 128, 1);
        case 256: FG64(256, 256, 1);  case 512: FG64(512, 512, 1);  default: FG64(1024, 1024, 1);
    }
#undef FG64
}

// scn_kernel<G, T> as scenario_dispatch (formation_hip.hip) chooses it: G = pow2 >= N + M lanes per env in workgroups of 64 threads,
// one env per workgroup of G threads beyond 64 entities; LDS by scn_lds_bytes.  a.stage = 1: the staged observation writer.
// -2: the workgroup's LDS (with the image, if asked for) does not fit; -4: the runtime refused; 0: launched
template <int G, int T>
static int launch_scn64(const ScnArgs& a, int obs_dim, hipStream_t st) {
    constexpr int E = scn_envs_per_group(G);
    static_assert(E == T / G, "the kernel's envs per workgroup");
    const int grid = (a.B + E - 1) / E;
    const long long lds = scn_lds_bytes(G, a.N, a.sc.num_landmarks, a.sc.num_obstacles, a.stage ? obs_dim : 0);
    if (lds > FG64_LDS_LIMIT) return -2;
    const auto kernel = &scn_kernel<G, T>;
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -4;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(T), (size_t)lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

}  // namespace fg

extern "C" {

// Constants in double, field for field what FgParams holds in float (include/formation_hip.h)
struct Fg64Params {
    double dt, damping, contact_force, contact_margin, sensitivity, mass, dist_min, collide_thresh;
    int32_t world_length, reserved;
};

// The World options of FgParams in double (u_noise stays 0: its draws are fp32 by design, distributional parity only)
struct Fg64Wall {
    int32_t vertical, soft;                 // FgWall.vertical / .soft
    double axis_pos, end0, end1, width;
};
struct Fg64Options {
    double accel, max_speed;                // 0 = None
    int32_t num_walls, reserved;
    Fg64Wall walls[FG_MAX_WALLS];
    const double* agent_props;              // DEVICE double [N][FG_AGENT_PROPS] (columns as FgParams.agent_props) or NULL
    const double* comm_state;               // DEVICE double [B][N][2] or NULL
};

static void fg64_args(fg::Args& a, const Fg64Params* params, int B, int N, int K) {
    memset(&a, 0, sizeof(a));
    a.p.dt = params->dt; a.p.damping = params->damping; a.p.contact_force = params->contact_force;
    a.p.contact_margin = params->contact_margin; a.p.sensitivity = params->sensitivity; a.p.mass = params->mass;
    a.p.dist_min = params->dist_min; a.p.collide_thresh = params->collide_thresh; a.p.world_length = params->world_length;
    a.B = B; a.N = N; a.inv_n = 1.0 / (double)N; a.K = K; a.obs_every = 1; a.do_phys = 1; a.do_post = 1;
    a.obs_pitch = 3LL * N * N;
}

// fg_step_hd in fp64: state, actions, formation and every output are double arrays of the fp32 entry point's shapes.
// Returns 0 or a negative code (-1 bad argument, -2 unsupported N, -4 HIP error).
int fg64_step_hd(const Fg64Params* params, int B, int N,
                 double* pos_x, double* pos_y, double* vel_x, double* vel_y,
                 const double* act, double* ideal_shape, double* ideal_vel, int32_t* step,
                 double* obs, double* reward, double* indiv_reward, uint8_t* done,
                 int32_t* near_lm, int32_t* near_ag, int32_t* hd_idx, void* stream) {
    using namespace fg;
    if (!params || B < 0 || !pos_x || !pos_y || !vel_x || !vel_y || !act || !ideal_shape || !ideal_vel || !step || !obs || !reward)
        return -1;
    if (N < 3 || N > 1024) return -2;
    if (B == 0) return 0;
    Args a; fg64_args(a, params, B, N, 1);
    a.px = pos_x; a.py = pos_y; a.vx = vel_x; a.vy = vel_y; a.act = act;
    a.shape = ideal_shape; a.ivel = ideal_vel; a.step = step;
    a.obs = obs; a.rew = reward; a.indiv = indiv_reward; a.done = done;
    a.near_lm = near_lm; a.near_ag = near_ag; a.hd_idx = hd_idx;
    return launch_step64(a, near_lm || near_ag || hd_idx, false, (hipStream_t)stream);
}

// fg_step_hd / the K-loop rollout of the World options in fp64: step_kernel's OPTS instantiation, K steps in ONE launch as the
// product runs option rollouts.  act [K][B][N][2], obs [K][B][N][6N], reward / indiv_reward / done [K][B][N]; the index outputs
// hold the last step's.  comm_state is read once per launch.  Returns 0, -1 bad argument, -2 unsupported N or a workgroup whose
// LDS does not fit the device, -4 HIP error.
int fg64_step_hd_opts(const Fg64Params* params, const Fg64Options* opts, int B, int N, int K,
                      double* pos_x, double* pos_y, double* vel_x, double* vel_y,
                      const double* act, double* ideal_shape, double* ideal_vel, int32_t* step,
                      double* obs, double* reward, double* indiv_reward, uint8_t* done,
                      int32_t* near_lm, int32_t* near_ag, int32_t* hd_idx, void* stream) {
    using namespace fg;
    if (!params || !opts || B < 0 || K < 1 || !pos_x || !pos_y || !vel_x || !vel_y || !act || !ideal_shape || !ideal_vel || !step ||
        !obs || !reward)
        return -1;
    if (opts->num_walls < 0 || opts->num_walls > FG_MAX_WALLS || opts->accel < 0 || opts->max_speed < 0) return -1;
    if (N < 3 || N > 1024) return -2;
    if (B == 0) return 0;
    Args a; fg64_args(a, params, B, N, K);
    a.p.accel = opts->accel; a.p.max_speed = opts->max_speed; a.p.u_noise = 0.0;
    a.p.num_walls = opts->num_walls;
    for (int w = 0; w < opts->num_walls; ++w) {
        const Fg64Wall& s = opts->walls[w];
        a.p.walls[w].vertical = s.vertical; a.p.walls[w].soft = s.soft;
        a.p.walls[w].axis_pos = s.axis_pos; a.p.walls[w].end0 = s.end0; a.p.walls[w].end1 = s.end1; a.p.walls[w].width = s.width;
    }
    a.p.agent_props = opts->agent_props; a.p.comm_state = opts->comm_state;
    a.coll_scale = params->collide_thresh / params->dist_min;           // divided in double
    a.px = pos_x; a.py = pos_y; a.vx = vel_x; a.vy = vel_y; a.act = act;
    a.shape = ideal_shape; a.ivel = ideal_vel; a.step = step;
    a.obs = obs; a.rew = reward; a.indiv = indiv_reward; a.done = done;
    a.near_lm = near_lm; a.near_ag = near_ag; a.hd_idx = hd_idx;
    return launch_step64(a, true, true, (hipStream_t)stream);
}

// fg_rollout_hd in fp64 for 9, 27, 81 and 243 agents (the reference's own hierarchy sizes): K steps in ONE launch of the pipelined kernel; act [K][B][N][2], obs [K][B][N][6N],
// reward / indiv_reward / done [K][B][N].  No auto-reset (the fixtures' episodes do not end inside a launch).
int fg64_rollout_hd(const Fg64Params* params, int B, int N, int K,
                    double* pos_x, double* pos_y, double* vel_x, double* vel_y,
                    const double* act, double* ideal_shape, double* ideal_vel, int32_t* step,
                    double* obs, double* reward, double* indiv_reward, uint8_t* done, void* stream) {
    using namespace fg;
    if (!params || B < 0 || K < 1 || !pos_x || !pos_y || !vel_x || !vel_y || !act || !ideal_shape || !ideal_vel || !step || !obs || !reward)
        return -1;
    if (N != 9 && N != 27 && N != 81 && N != 243) return -2;
    if (B == 0) return 0;
    Args a; fg64_args(a, params, B, N, K);
    a.px = pos_x; a.py = pos_y; a.vx = vel_x; a.vy = vel_y; a.act = act;
    a.shape = ideal_shape; a.ivel = ideal_vel; a.step = step;
    a.obs = obs; a.rew = reward; a.indiv = indiv_reward; a.done = done;
    hipStream_t st = (hipStream_t)stream;
    const hipError_t err = N == 9 ? launch_roll64<9, 16, 64, 128, 4>(a, st) : N == 27 ? launch_roll64<27, 32, 128, 256, 4>(a, st)
                         : N == 81 ? launch_wide64<81, 2, 2, 128>(a, st) : launch_wide64<243, 4, 1, 256>(a, st);
    return err == hipSuccess ? 0 : -4;
}

// fg_rollout_hd_returns in fp64: the discounted returns of C candidate action sequences from the current state, ONE launch of
// returns_kernel<N, G, 256> at the product's (N, G) table (returns_dispatch's FG_RETURNS list).  The state is read only.
// act [C][K][B][N][2], ret / indiv_ret [C][B][N] (indiv_ret may be NULL), steps [B] (may be NULL).
// Returns 0, -1 bad argument, -2 unsupported N, -4 HIP error; an empty batch is 0 without a launch.
int fg64_rollout_hd_returns(const Fg64Params* params, int B, int N, int K, int C, double gamma,
                            const double* pos_x, const double* pos_y, const double* vel_x, const double* vel_y,
                            const double* ideal_shape, const double* ideal_vel, const int32_t* step,
                            const double* act, double* ret, double* indiv_ret, int32_t* steps, void* stream) {
    using namespace fg;
    if (!params || B < 0 || K < 1 || C < 1 || !(gamma >= 0.0 && gamma <= 1.0) || (long long)B * C > 0x7fffffffLL) return -1;
    if (N != 3 && N != 4 && N != 8 && N != 9 && N != 16 && N != 25 && N != 27 && N != 32) return -2;
    if (B == 0) return 0;
    if (!pos_x || !pos_y || !vel_x || !vel_y || !ideal_shape || !ideal_vel || !step || !act || !ret) return -1;
    ReturnsArgs a; memset(&a, 0, sizeof(a));
    a.p.dt = params->dt; a.p.damping = params->damping; a.p.contact_force = params->contact_force;
    a.p.contact_margin = params->contact_margin; a.p.sensitivity = params->sensitivity; a.p.mass = params->mass;
    a.p.dist_min = params->dist_min; a.p.collide_thresh = params->collide_thresh; a.p.world_length = params->world_length;
    a.B = B; a.K = K; a.C = C; a.gamma = gamma;
    a.px = pos_x; a.py = pos_y; a.vx = vel_x; a.vy = vel_y; a.shape = ideal_shape; a.ivel = ideal_vel; a.step = step;
    a.act = act; a.ret = ret; a.indiv_ret = indiv_ret; a.steps = steps;
    hipStream_t st = (hipStream_t)stream;
#define FG64_RETURNS(NN, G) if (N == NN) return launch_returns64<NN, G>(a, st);
    FG64_RETURNS(3, 4) FG64_RETURNS(4, 4) FG64_RETURNS(8, 8) FG64_RETURNS(9, 16) FG64_RETURNS(16, 16)
    FG64_RETURNS(25, 32) FG64_RETURNS(27, 32) FG64_RETURNS(32, 32)
#undef FG64_RETURNS
    return -2;
}

// The landmark scenarios' constants in double, field for field what FgScenario holds (kind: FG_SCN_BASIC ... FG_SCN_OBSTACLE)
struct Fg64Scenario {
    int32_t kind, num_landmarks, num_obstacles, num_obs;
    double obs_range, obstacle_size, obstacle_vx, obstacle_vy, obstacle_floor, penalty;
};

// fg_step_scenario / fg_step_basic / fg_rollout_scenario in fp64: K steps in ONE launch of scn_kernel through its own K-loop (K = 1:
// a single step; do_physics = 0: the observation and rewards of the state as it is).  opts: accel, max_speed, walls and the per-agent
// table (comm_state must be NULL).  act [K][B][N][2], landmarks [B][L][2], obst_pos / obst_vel [B][M][2], obs [K / obs_every][B][N][D],
// reward / indiv_reward / done [K][B][N], near_ag [K][B][L] (basic; may be NULL).  stage: 0 = every lane writes its row straight to
// memory, 1 = the rows are composed in LDS and streamed out (the product picks this where the image fits 48 KB).  auto_reset, u_noise
// and comm_state stay off.  Returns 0, -1 bad argument, -2 unsupported count or a workgroup whose LDS does not fit (stage = 1 with
// an image that does not fit included), -4 HIP error.
int fg64_rollout_scenario(const Fg64Params* params, const Fg64Scenario* sc, const Fg64Options* opts, int B, int N, int K,
                          int do_physics, int obs_every, int stage,
                          double* pos_x, double* pos_y, double* vel_x, double* vel_y, const double* act, double* landmarks,
                          double* obst_pos, double* obst_vel, int32_t* step,
                          double* obs, double* reward, double* indiv_reward, uint8_t* done, int32_t* near_ag, void* stream) {
    using namespace fg;
    if (!params || !sc || !opts || B < 0 || K < 1 || obs_every < 1 || (K > 1 && !do_physics) || (stage != 0 && stage != 1)) return -1;
    if (!pos_x || !pos_y || !vel_x || !vel_y || !landmarks || !obs || (do_physics && (!act || !reward))) return -1;
    if (sc->kind < FG_SCN_BASIC || sc->kind > FG_SCN_OBSTACLE || sc->num_landmarks < 1 || sc->num_obstacles < 0) return -1;
    if ((sc->kind == FG_SCN_OBSTACLE) != (sc->num_obstacles > 0) || (sc->num_obstacles > 0 && (!obst_pos || !obst_vel))) return -1;
    if (opts->num_walls < 0 || opts->num_walls > FG_MAX_WALLS || opts->accel < 0 || opts->max_speed < 0 || opts->comm_state) return -1;
    if (sc->kind == FG_SCN_PARTIAL && (sc->num_obs < 0 || sc->num_obs > 1024)) return -1;
    if (N < 1 || N + sc->num_obstacles > 1024 || sc->num_landmarks > 1024) return -2;
    if (B == 0) return 0;
    ScnArgs a; memset(&a, 0, sizeof(a));
    a.p.dt = params->dt; a.p.damping = params->damping; a.p.contact_force = params->contact_force;
    a.p.contact_margin = params->contact_margin; a.p.sensitivity = params->sensitivity; a.p.mass = params->mass;
    a.p.dist_min = params->dist_min; a.p.collide_thresh = params->collide_thresh; a.p.world_length = params->world_length;
    a.p.accel = opts->accel; a.p.max_speed = opts->max_speed; a.p.u_noise = 0.0;
    a.p.num_walls = opts->num_walls;
    for (int w = 0; w < opts->num_walls; ++w) {
        const Fg64Wall& s = opts->walls[w];
        a.p.walls[w].vertical = s.vertical; a.p.walls[w].soft = s.soft;
        a.p.walls[w].axis_pos = s.axis_pos; a.p.walls[w].end0 = s.end0; a.p.walls[w].end1 = s.end1; a.p.walls[w].width = s.width;
    }
    a.p.agent_props = opts->agent_props;
    a.sc.kind = sc->kind; a.sc.num_landmarks = sc->num_landmarks; a.sc.num_obstacles = sc->num_obstacles; a.sc.num_obs = sc->num_obs;
    a.sc.obs_range = sc->obs_range; a.sc.obstacle_size = sc->obstacle_size; a.sc.obstacle_vx = sc->obstacle_vx;
    a.sc.obstacle_vy = sc->obstacle_vy; a.sc.obstacle_floor = sc->obstacle_floor; a.sc.penalty = sc->penalty;
    a.B = B; a.N = N; a.do_phys = do_physics ? 1 : 0; a.K = K; a.obs_every = obs_every; a.stage = stage;
    a.inv_n = 1.0 / (double)N; a.inv_l = 1.0 / (double)sc->num_landmarks;
    a.coll_scale = params->collide_thresh / params->dist_min;           // divided in double
    a.px = pos_x; a.py = pos_y; a.vx = vel_x; a.vy = vel_y; a.act = act; a.lm = landmarks; a.opos = obst_pos; a.ovel = obst_vel;
    a.step = step; a.obs = obs; a.rew = reward; a.indiv = indiv_reward; a.done = done; a.near_ag = near_ag;
    const int nbr = sc->kind == FG_SCN_PARTIAL ? sc->num_obs : N - 1;
    const int D = scn_obs_dim(sc->kind, N, sc->num_landmarks, sc->num_obstacles, nbr);
    hipStream_t st = (hipStream_t)stream;
    switch (scn_group_lanes(N + sc->num_obstacles)) {
        case 4: return launch_scn64<4, FG_SCN_T>(a, D, st);       case 8: return launch_scn64<8, FG_SCN_T>(a, D, st);
        case 16: return launch_scn64<16, FG_SCN_T>(a, D, st);     case 32: return launch_scn64<32, FG_SCN_T>(a, D, st);
        case 64: return launch_scn64<64, FG_SCN_T>(a, D, st);     case 128: return launch_scn64<128, 128>(a, D, st);
        case 256: return launch_scn64<256, 256>(a, D, st);        case 512: return launch_scn64<512, 512>(a, D, st);
        default: return launch_scn64<1024, 1024>(a, D, st);
    }
}

}  // extern "C"
