/*
 * formation_hip.h - C ABI of libformation_hip.so, the MI355X (gfx950) native
 * implementation of the formation_gym hot path.
 *
 * The reference (jc-bao/gym-formation) is pure Python and has no FFI; its
 * boundary for this path is the plugin API
 *     formation_gym.make_env(...)                 formation_gym/__init__.py:6-17
 *     MultiAgentEnv.reset() / .step(action_n)     formation_gym/environment.py:113-156
 *     Scenario.{reset_world,observation,reward}   formation_gym/envs/formation_hd_env.py:38-95
 *     World.step()                                formation_gym/core.py:206-225
 * Each entry point below names the reference interface it replaces.  The host
 * side that binds them through ctypes is gym-formation_amd/formation_gym/_native.py;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer owned by the caller
 *     (e.g. torch.Tensor.data_ptr()); the library allocates nothing persistent
 *     and keeps no pointer after a call returns.
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as
 *     void*, NULL = the default stream); no device synchronisation inside, so
 *     every entry point may be captured into a hipGraph.
 *   - return value: FG_OK (0) or a negative FgStatus; nothing throws or exits.
 *     An empty batch (B = 0), zero steps (K = 0) or count = 0 is a successful no-op:
 *     no launch, buffers may be NULL.
 *     fg_last_error() returns a thread-local description of the last failure.
 *   - layouts are env-major and contiguous.  B = number of independent
 *     environments (the data-parallel unit), N = agents per environment.
 *       pos_x,pos_y,vel_x,vel_y  float [B][N]     structure-of-arrays agent state
 *       act                      float [B][N][2]  raw actions (scaled by `sensitivity` inside)
 *       ideal_shape              float [B][N][2]  Scenario.ideal_shape (already centred)
 *       ideal_vel                float [B][2]     Scenario.ideal_vel
 *       step                     int32 [B]        MultiAgentEnv.current_step per env
 *       obs                      float [B][N][6N] (16-byte aligned base)
 *       reward                   float [B][N]     shared reward, broadcast to every agent
 *       indiv_reward             float [B][N]     info_n[i]['individual_reward']   (may be NULL)
 *       done                     uint8 [B][N]     current_step >= world_length
 *       near_lm, near_ag         int32 [B][N]     landmark-index assignments        (may be NULL)
 *       hd_idx                   int32 [B][4]     Hausdorff witness indices         (may be NULL)
 */
#ifndef FORMATION_HIP_H_
#define FORMATION_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FG_ABI_VERSION 8
#define FG_MAX_AGENTS 1024
#define FG_MAX_WALLS 4

typedef enum FgStatus {
    FG_OK = 0,
    FG_ERR_BAD_ARG = -1,        /* NULL pointer, B < 0, K < 0, bad params              */
    FG_ERR_UNSUPPORTED_N = -2,  /* N < 2 or N > FG_MAX_AGENTS                          */
    FG_ERR_ALIGNMENT = -3,      /* obs base not 16-byte aligned                        */
    FG_ERR_HIP = -4             /* a HIP runtime call failed (see fg_last_error)       */
} FgStatus;

/* Physics / scenario constants.  Field -> reference source:
 *   dt              core.py:125            damping         core.py:127
 *   contact_force   core.py:129            contact_margin  core.py:130
 *   sensitivity     environment.py:218-221 mass            core.py:69,73-75
 *   dist_min        core.py:307 (size_a + size_b, force contact distance)
 *   collide_thresh  formation_hd_env.py:121 ((size_a+size_b)/2) or
 *                   basic_formation_env.py:91 (size_a+size_b)
 *   world_length    formation_hd_env.py:13,16 / core.py:113
 *   auto_reset      0: like the reference env (caller resets);
 *                   1: vec-env worker semantics, train/maddpg-v2/utils/env_wrappers.py:14-18
 *                      (when done: re-initialise the env on device and return the RESET
 *                      observation together with the pre-reset reward/done)
 *   seed, rng_offset  counter-RNG key / per-call offset for the device-side reset
 *                   (distributional parity with formation_hd_env.py:77-95 only).
 *                   The contract, pinned draw by draw by tests/test_gpu_counter_rng.py against tests/counter_rng.py:
 *                   every draw is ONE Philox4x32-10 block with key {lo32(seed), hi32(seed)} and counter
 *                   {env_index_base + b, stream code, lo32(off), hi32(off)}, off = rng_offset + *rng_offset_dev (+ k at
 *                   step k of a K-step launch, a 64-bit sum).  Stream codes (counter word 1) and the words used:
 *                     formation_hd_env reset, agent i     i                      c0,c1 -> position; c2,c3 -> ideal shape
 *                                                                                 before centring (shape = raw - sum / N)
 *                     ... its ideal velocity              0xFFFFFFFF             c0,c1
 *                     landmark-scenario reset: agent i    i                      c0,c1
 *                                  landmark l / obstacle k  0x10000000 | l / 0x20000000 | k     c0,c1
 *                     motor noise (u_noise), agent i      i ^ 0x80000000         c0,c1 -> Box-Muller
 *                     comm noise (c_noise), agent i,      (i | 0x40000000 | q << 12) ^ 0x80000000   c0,c1 -> Box-Muller
 *                       components 2q, 2q + 1
 *                     actor exploration, agent i          (i | 0x20000000) ^ 0x80000000             c0,c1 -> Box-Muller
 *                   uniform: u = (c >> 8) * 2^-23 - 1 in [-1, 1), exact in fp32; Box-Muller: r = sqrt(-2 ln(((c0 >> 8) + 1)
 *                   / 2^24)), a = 6.2831853f * (c1 >> 8) / 2^24, (r cos a, r sin a).  Disjoint for i, l, k < 1024, q < 2^16.
 * World options that no reference scenario switches on (0 = None, the reference default):
 *   accel           core.py:236 + environment.py:219-220: force = mass*accel*(accel*action)
 *   max_speed       core.py:271-276 speed clamp after the velocity update
 *   u_noise         core.py:232-233 Gaussian motor noise (device counter RNG, distributional parity)
 *   walls           core.py:27-41,255-261,325-362 get_wall_collision_force; hard or soft (FgWall.soft)
 * Layout option of the observation output (fg_step_hd, fg_observe_hd, fg_rollout_hd, fg_rollout_hd_policy):
 *   obs_env_pitch   the [N][6N] block of env b starts obs_env_pitch floats after env b-1's (even, >= 6 N^2);
 *                   every agent count of the reference is odd, so contiguous env blocks are only 8-byte aligned -
 *                   a pitch rounded up to 32 floats puts every env on its own 128-byte lines (a strided
 *                   [B][N][6N] view on the caller's side).  A rollout's step slots are B * pitch apart.  The pad
 *                   floats between env blocks belong to the library: they may be overwritten with zeros.      */
typedef struct FgWall {
    int32_t vertical;    /* orient: 0 = 'H' (lies on y = axis_pos), 1 = 'V' */
    float axis_pos;
    float end0, end1;    /* endpoints along the wall */
    float width;
    int32_t soft;        /* core.py:36-37 Wall.hard: 0 = hard (every entity feels it), 1 = soft (ghost entities pass through, :326-327) */
} FgWall;

typedef struct FgParams {
    float dt;
    float damping;
    float contact_force;
    float contact_margin;
    float sensitivity;
    float mass;
    float dist_min;
    float collide_thresh;
    int32_t world_length;
    int32_t auto_reset;
    uint64_t seed;
    uint64_t rng_offset;
    float accel;
    float max_speed;
    float u_noise;
    int32_t num_walls;
    FgWall walls[FG_MAX_WALLS];
    int32_t obs_env_pitch;   /* floats between the observation blocks of consecutive envs; 0 = 6 N^2 (contiguous) */
    int32_t env_index_base;  /* GLOBAL index of this batch's env 0 (a rank's slice of a sharded batch): the device
                                counter RNG (auto-reset, fg_reset_hd, motor noise) is keyed by seed and GLOBAL env index,
                                so its draws do not depend on how the batch is cut over GPUs */
    const uint64_t* rng_offset_dev;  /* optional DEVICE counter added to rng_offset when the launch runs (NULL = none): a
                                caller that replays a captured hipGraph keeps its per-step offset here and advances it
                                with a device-side add between launches, since by-value arguments are frozen in a graph.
                                The library only reads it. */
    const float* agent_props;  /* optional DEVICE table float [N][FG_AGENT_PROPS], one row per agent (NULL = every agent
                                takes the scalars above - all the reference's scenarios):
                                  [0] mass       Entity.initial_mass, core.py:68-75: contact forces are scaled by
                                                 force_ratio = m_b / m_a (core.py:314-317), velocity gains F / m (:270)
                                  [1] size       Entity.size: contact distance of a pair = size_a + size_b (core.py:307),
                                                 collision penalty distance = collide_thresh / dist_min * (size_a + size_b)
                                                 (formation_hd_env.py:119-121), wall contact (core.py:340-344)
                                  [2] accel      Entity.accel (0 = None): core.py:236, environment.py:219-220
                                  [3] max_speed  Entity.max_speed (0 = None): core.py:271-276
                                  [4] u_noise    Agent.u_noise (0 = None): core.py:232-233
                                  [5] c_noise    Agent.c_noise for fg_update_comm (0 = None; < 0 = a silent agent)
                                  [6] flags      an integer stored as a float, 0 for an ordinary agent:
                                                 1 = not movable (core.py:231, 266-267: no action force, state never
                                                     integrated; a partner's contact force is then not scaled by the mass
                                                     ratio, :319-321),
                                                 2 = does not collide (:292-293: no contact force with anybody; the reward's
                                                     collision penalties of such an agent are not counted,
                                                     formation_hd_env.py:71),
                                                 4 = ghost (passes through soft walls, :326-327)
                                  [7] reserved (0)
                                With a table, `sensitivity` is the value for agents whose accel is None (5.0) and
                                mass / dist_min / accel / max_speed / u_noise above are not read.  Honoured by
                                fg_step_hd, fg_physics_step, fg_observe_hd, fg_rollout_hd, fg_rollout_hd_policy, and - columns
                                [0] ... [4] and [6], the agents only: obstacles keep FgScenario.obstacle_size, unit mass and
                                are ordinary movable colliders - by fg_step_scenario, fg_step_basic, fg_rollout_scenario
                                (penalty distance of a pair = collide_thresh / dist_min * (size_a + size_b)). */
    const float* comm_state;   /* optional DEVICE float [B][N][2] = AgentState.c of every agent (World.dim_c = 2): copied
                                into the communication block of the observation, row i = c_j for j != i in index order
                                (formation_hd_env.py:48-51,59); NULL = zeros, the silent agents of every reference
                                scenario (core.py:281-282).  Honoured by fg_step_hd, fg_observe_hd, fg_rollout_hd. */
    int32_t obs_placed;        /* hint: 1 = the observation buffer of this launch was composed with fg_arena_* of chunks spread
                                over the device's memory.  Such a buffer takes the store stream of MORE writer
                                waves: the 27-agent rollout then runs 8 paced writer waves per workgroup (11.7 us/step at
                                27 x 4096) where 4 are best on an ordinary allocation (12.9 there, 13.2-14.4 with 8).  0 = unknown */
    int32_t obs_zero_primed;   /* promise: 1 = in the fp32 observation buffer of this launch, units [N, 2N-1) of every row of every
                                env block it writes - the communication block, zeros while comm_state is NULL - ALREADY hold
                                zeros (the caller filled the buffer with zeros once, and since then only launches without
                                comm_state have written it).  The 16-32-agent tile writers of fg_rollout_hd /
                                fg_rollout_hd_policy then leave out the stores of whole 128-byte lines (by device address)
                                that lie wholly inside one row's block: 13.6 % of the observation bytes at 27 agents.  Every
                                other kernel, and any launch with comm_state, ignores it and writes everything.  The buffer's
                                contents after the launch are the same either way.  0 = no promise (was reserved0: a caller that
                                zero-fills FgParams keeps today's behaviour). */
} FgParams;
#define FG_AGENT_PROPS 8
#define FG_AGENT_IMMOVABLE 1
#define FG_AGENT_NO_COLLIDE 2
#define FG_AGENT_GHOST 4
#define FG_AGENT_SCRIPTED 8   /* the action of this agent is a scripted agent's `action.u` (Agent.action_callback, core.py:210-211):
                                 taken as it is - environment.py:216-221's sensitivity scaling applies to policy agents only */

/* Landmark scenarios with few agents (fg_step_scenario).  Field -> reference source:
 *   kind            which Scenario file under formation_gym/envs/
 *   num_landmarks   L: make_world default of that file (make_env passes only num_agents)
 *   num_obstacles   M: formation_hd_obs_env.py:14 (movable colliding landmarks)
 *   num_obs         formation_hd_partial_env.py:15,44 ring neighbours observed
 *   obs_range       formation_hd_partial_range_env.py:15,46 clip of relative positions
 *   obstacle_size   formation_hd_obs_env.py:39;  obstacle_v{x,y}, obstacle_floor  :84-89
 *   penalty         reward per collision: 1 (basic/partial/range), 2 (obstacle, :92-98)
 * At the reference's own shapes - basic (N, L) = (3, 3), partial (5, 5, num_obs 3), range (4, 4), obstacle (4, 4, M 3), and
 * what make_env's default num_agents = 3 makes of the last three - a launch runs the one-env-per-lane kernel
 * (csrc/fg_scn_lane_kernel.hpp: every count a compile-time constant), else the run-time-count kernel; same results.   */
typedef enum FgScenarioKind {
    FG_SCN_BASIC = 1, FG_SCN_PARTIAL = 2, FG_SCN_RANGE = 3, FG_SCN_OBSTACLE = 4
} FgScenarioKind;

typedef struct FgScenario {
    int32_t kind;
    int32_t num_landmarks;
    int32_t num_obstacles;
    int32_t num_obs;
    float obs_range;
    float obstacle_size;
    float obstacle_vx;
    float obstacle_vy;
    float obstacle_floor;
    float penalty;
    int32_t variant;         /* 0 = the library's choice of kernel; 1 = the run-time-count kernel even where a
                                one-env-per-lane instantiation exists (tests / A-B runs: the two agree bit for bit) */
    int32_t reserved;
} FgScenario;

/* Placed device memory ------------------------------------------------------
 * The rate at which the rollout kernels stream observations depends on WHICH physical memory the buffer is composed of: a
 * multi-GB buffer on physically neighbouring memory runs the same launch at 5.0-5.4 TB/s, a well composed one at 6.2-6.8
 * TB/s (a physically contiguous allocation: 2-2.6 TB/s; profiles/r03_place/).  Which composition is fast cannot be told in
 * advance (the driver decides where a chunk lies; compositions made by rule do not hold up: profiles/r04_place/), so a caller
 * TIMES its own launch on a few compositions and keeps the best - from an arena that need not be larger than 1.5-6 x the
 * buffer (profiles/r04_place/arena_size.txt).  An arena is a set of separately created physical chunks (HIP virtual memory
 * management) from which a caller composes buffers:
 *   fg_arena_create   creates ceil(bytes / chunk) chunks of device memory on `device` (chunk_bytes is rounded up to the
 *                     allocation granularity; 0 = 1 GiB) and gives them their place in memory in INDEX order (a chunk is
 *                     placed when it is first mapped, so every chunk is mapped once and unmapped again: chunks far apart
 *                     in index lie far apart in memory); on return nothing is mapped.  *chunk_out = chunk size,
 *                     *chunks_out = count
 *   fg_arena_map      maps `count` chunks (indices, any order) at fresh contiguous addresses *base, read-write for the
 *                     device: a buffer made of exactly those chunks.  A chunk is mapped at ONE address at a time
 *   fg_arena_unmap    removes one such mapping (its chunks become available again; their contents stay)
 *   fg_arena_trim     hands every chunk that is not mapped right now back to the driver
 *   fg_arena_destroy  unmaps and releases everything
 * unmap / destroy drain the device first (no launch may still be using the addresses); map returns when the mapping is
 * usable.  An address range that has held a mapping is never used again in this process: hipMemUnmap leaves the GPU's
 * translations of it behind on this stack (profiles/r03_place/va_reuse_check.txt), so the library retires the reservation
 * instead of freeing it - that costs address space only (fg_arena_retired_address_bytes: the running total; a placement of
 * a 1.4 GB buffer retires ~250 GB of the 128 TiB; once 64 TiB are retired fg_arena_create / _map refuse with FG_ERR_HIP and the
 * caller uses ordinary allocations), the physical memory goes back at trim / destroy.
 * These are the only entry points that allocate; they enqueue nothing and take no stream.  Calls on ONE arena must not
 * run concurrently (the arena is the caller's object; different arenas are independent). */
int fg_arena_create(int device, uint64_t bytes, uint64_t chunk_bytes, void** arena, uint64_t* chunk_out, uint32_t* chunks_out);
int fg_arena_map(void* arena, const uint32_t* chunk_index, uint32_t count, void** base);
int fg_arena_unmap(void* arena, void* base);
/* shrinks the mapping at `base` to chunks [first, first + count) of it (the others are unmapped, their addresses retired); the
 * window keeps its address, returned in *new_base = base + first * chunk */
int fg_arena_keep_window(void* arena, void* base, uint32_t first, uint32_t count, void** new_base);
int fg_arena_trim(void* arena);
uint64_t fg_arena_retired_address_bytes(void);
int fg_arena_destroy(void* arena);

/* library / diagnostics --------------------------------------------------- */
int fg_abi_version(void);
const char* fg_last_error(void);
/* The device an entry point would launch on for this stream and this first state pointer: the stream's device when the
 * stream is not NULL, else the device the pointer's memory lives on (hipPointerGetAttributes), else -1 = "cannot tell: the
 * calling thread's current device".  Every entry point applies this rule (and switches device for the duration of the call
 * when the process sees more than one GPU), so that an env living on cuda:1 can be driven from a thread whose current device
 * is cuda:0; this call only reports it.  Memory composed with fg_arena_map counts as the device's like any other allocation
 * (tests/test_gpu_multidevice.py::test_launch_device_rule_on_one_gpu). */
int fg_launch_device(void* stream, const void* data);
/* Launch geometry the library will use for N agents: threads per workgroup,
 * environments per workgroup, dynamic LDS bytes.  Returns FgStatus. */
int fg_kernel_config(int N, int* threads, int* envs_per_wg, int* lds_bytes);
/* Dry run of the dispatch: which kernel instantiation(s) and launch geometry fg_step_hd (K = 0), fg_rollout_hd (K >= 1,
 * per_layer = 0), fg_rollout_hd_policy (per_layer > 0) or - with a scenario descriptor - fg_rollout_scenario would use for this
 * shape and these params (obs_env_pitch, obs_placed, World options and all), written to `out` as text.  Touches no device:
 * callable without a GPU.  tests/test_dispatch_snapshot.py holds the committed choices over a grid of shapes. */
int fg_describe_launch(const FgParams* params, const FgScenario* scenario, int B, int N, int K, int per_layer, int obs_every,
                       int index_outputs, char* out, int out_len);
/* Algorithmic bytes per env-step of fg_step_hd (24 N^2 + 53 N + 16). */
int64_t fg_step_hd_bytes(int N);

/* MultiAgentEnv.step for formation_hd_env, all B envs, ONE fused launch (more than 64 agents in at most 128 envs: two
 * launches - everything but the observation, then the observation streamed by several workgroups per env; same results):
 * _set_action (environment.py:187-236) -> World.step (core.py:206-225:
 * apply_action_force :228-237, apply_environment_force :240-262 with
 * get_entity_collision_force :289-322, integrate_state :264-277,
 * update_agent_state :279-286) -> Scenario.observation / reward / done for every
 * agent (formation_hd_env.py:38-75, environment.py:126-138,172-178).
 * State (pos/vel/step, and ideal_shape/ideal_vel when auto_reset) is updated in place. */
int fg_step_hd(const FgParams* params, int B, int N,
               float* pos_x, float* pos_y, float* vel_x, float* vel_y,
               const float* act, float* ideal_shape, float* ideal_vel, int32_t* step,
               float* obs, float* reward, float* indiv_reward, uint8_t* done,
               int32_t* near_lm, int32_t* near_ag, int32_t* hd_idx, void* stream);

/* The same step as a PLAN: fg_step_hd_plan checks the arguments once and keeps the launch description (the pointers are the
 * caller's and must stay valid while the plan lives - like fg_arena_*, a declared exception to "keeps no pointer");
 * fg_plan_launch(plan, rng_offset) enqueues one step on the plan's stream with FgParams.rng_offset = rng_offset and nothing
 * else changed; fg_plan_destroy frees the description.  For step loops that re-use their buffers (MultiAgentEnv.step called
 * per step, environment.py:113-142, test.py:17-28): the per-step host work is a two-argument call plus the kernel launch.
 * Results equal fg_step_hd's bit for bit (the same dispatch). */
int fg_step_hd_plan(const FgParams* params, int B, int N,
                    float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                    const float* act, float* ideal_shape, float* ideal_vel, int32_t* step,
                    float* obs, float* reward, float* indiv_reward, uint8_t* done,
                    int32_t* near_lm, int32_t* near_ag, int32_t* hd_idx, void* stream, void** plan);
int fg_plan_launch(void* plan, uint64_t rng_offset);
int fg_plan_destroy(void* plan);

/* World.step only (core.py:206-225) incl. the action scaling of
 * environment.py:216-221; for per-stage parity tests.  Updates pos/vel in place. */
int fg_physics_step(const FgParams* params, int B, int N,
                    float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                    const float* act, void* stream);

/* Scenario.observation + Scenario.reward + _get_done on the CURRENT state, no
 * physics and no step increment (formation_hd_env.py:38-75; what env.reset()
 * returns, environment.py:154-155).  reward/indiv_reward/done may be NULL. */
int fg_observe_hd(const FgParams* params, int B, int N,
                  const float* pos_x, const float* pos_y, const float* vel_x, const float* vel_y,
                  const float* ideal_shape, const float* ideal_vel, const int32_t* step,
                  float* obs, float* reward, float* indiv_reward, uint8_t* done,
                  int32_t* near_lm, int32_t* near_ag, int32_t* hd_idx, void* stream);

/* K consecutive env.step calls in ONE launch (the caller's rollout loop,
 * test.py:17-28 / train/maddpg-v2/main.py:77-91) with pre-staged actions.
 *   act_seq [K][B][N][2]; obs_seq [K][B][N][6N]; reward_seq, indiv_seq [K][B][N];
 *   done_seq [K][B][N].  If obs_every > 1 only steps k with (k+1) % obs_every == 0
 *   write an observation (into slot k / obs_every); rewards/dones are always written. */
int fg_rollout_hd(const FgParams* params, int B, int N, int K,
                  float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                  const float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                  float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq,
                  int obs_every, void* stream);

/* Scenario.reset_world on device for the envs whose mask byte is non-zero
 * (mask NULL = all), counter-based RNG (formation_hd_env.py:77-95 draw
 * distribution: pos ~ U(-1,1)^2, vel = 0, ideal_shape = centred U(-1,1)^2,
 * ideal_vel ~ U(-1,1)^2, step = 0). */
int fg_reset_hd(const FgParams* params, int B, int N, const uint8_t* mask,
                float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                float* ideal_shape, float* ideal_vel, int32_t* step, void* stream);

/* The same reset drawn from each env's own legacy NumPy MT19937 stream (environment.py:106-110
 * np.random.seed; formation_hd_env.py:77-95 draw order), bit-exact with the reference's host RNG:
 *   mt_state uint32 [B][626] = RandomState.get_state() key[624], pos, pad; advanced in place.
 *   landmark_pos float [B][N][2] (may be NULL) receives the un-centred landmark positions. */
int fg_reset_hd_mt(int B, int N, const uint8_t* mask, uint32_t* mt_state,
                   float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                   float* ideal_shape, float* ideal_vel, float* landmark_pos, int32_t* step, void* stream);

/* The vec-env worker's reset (train/maddpg-v2/utils/env_wrappers.py:14-18: `if all(done): ob = env.reset()`) decided ON
 * THE DEVICE: every env whose episode is over (step[b] >= world_length) is re-initialised from its own MT19937 stream as
 * fg_reset_hd_mt does, and - if obs is not NULL - its block of the observation tensor [B][N][6N] (env blocks
 * obs_env_pitch floats apart, 0 = contiguous) is overwritten with the RESET observation (formation_hd_env.py:52-59 on the
 * fresh state, the bits fg_observe_hd gives).  No mask upload, no host read-back, one launch. */
int fg_reset_hd_mt_done(int B, int N, int world_length, uint32_t* mt_state,
                        float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                        float* ideal_shape, float* ideal_vel, float* landmark_pos, int32_t* step,
                        float* obs, int64_t obs_env_pitch, void* stream);

/* Scenario.reset_world of the landmark scenarios (basic_formation_env.py:54-65, formation_hd_partial_env.py:88-99,
 * formation_hd_partial_range_env.py:76-87, formation_hd_obs_env.py:101-120) continued on the device from each env's own legacy
 * NumPy MT19937 stream (mt_state uint32 [B][626] as for fg_reset_hd_mt): N agent positions, num_landmarks landmark positions,
 * num_obstacles obstacles from uniform([s_k, 2.0], [s_k+1, 2.5]) with the scenario's obstacle velocity - bit-exact with the
 * reference's draws.  Which envs: mask bytes (mask != NULL), every env (mask NULL, world_length <= 0), or the vec-env
 * worker's rule step[b] >= world_length (mask NULL, world_length > 0; env_wrappers.py:14-18). */
int fg_reset_scenario_mt(const FgScenario* scenario, int B, int N, const uint8_t* mask, int world_length, uint32_t* mt_state,
                         float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                         float* landmarks, float* obst_pos, float* obst_vel, int32_t* step, void* stream);

/* World.update_agent_state (core.py:279-286) for all B x N agents: state.c = action.c + c_noise * N(0,1) for a
 * non-silent agent, zeros for a silent one (agent_props[i][5] < 0; without a table every agent is non-silent and
 * noise-free).  dim_c = 2.  action_c, comm_state float [B][N][2]; the noise comes from the device counter RNG
 * (seed, env_index_base + b, agent, rng_offset: distributional parity, the reference draws np.random.randn). */
int fg_update_comm(const FgParams* params, int B, int N, const float* action_c, float* comm_state, void* stream);
/* The same for any World.dim_c (core.py:279-286 takes whatever the World says): action_c, comm_state float [B][N][dim_c].
 * dim_c = 2 is fg_update_comm itself; the fused formation_hd_env kernels read a communication block of dim_c = 2 only
 * (FgParams.comm_state), other widths serve the World API (World.step / update_agent_state). */
int fg_update_comm_dim(const FgParams* params, int B, int N, int dim_c, const float* action_c, float* comm_state, void* stream);

/* MultiAgentEnv.step for basic_formation_env (BASELINE config 1):
 * same physics; observation basic_formation_env.py:29-41, reward :43-52.
 *   landmarks float [B][L][2]; obs float [B][N][4 + 2L + 4(N-1)].
 * params->auto_reset: as for fg_step_scenario below. */
int fg_step_basic(const FgParams* params, int B, int N, int L, int do_physics,
                  float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                  const float* act, float* landmarks, int32_t* step,
                  float* obs, float* reward, float* indiv_reward, uint8_t* done,
                  int32_t* near_ag, void* stream);

/* MultiAgentEnv.step for formation_hd_partial_env / formation_hd_partial_range_env /
 * formation_hd_obs_env (and basic_formation_env), N + M <= 1024 (one env per lane group of a wave up to 64 entities,
 * per workgroup beyond):
 *   landmarks float [B][L][2]; obst_pos, obst_vel float [B][M][2] (updated in place, NULL if M = 0);
 *   obs float [B][N][D], D = 2 (+2 basic) + 2L + 2M + 2*nbr + 2(N-1), nbr = num_obs (partial) or N-1.
 * do_physics = 0 evaluates observation/reward/done on the current state (env.reset()).
 * params->auto_reset (with do_physics): the vec-env worker's rule inside the launch (env_wrappers.py:14-18) - an env whose
 * step counter reaches world_length restarts at once: agents, landmarks and obstacles are re-drawn exactly as
 * fg_reset_scenario draws them (same counter RNG: seed, env_index_base + b, rng_offset), step = 0, and the observation
 * written is the RESET observation while reward / indiv_reward / done keep the finished step's values.  `landmarks` is
 * written only then. */
int fg_step_scenario(const FgParams* params, const FgScenario* scenario, int B, int N, int do_physics,
                     float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                     const float* act, float* landmarks, float* obst_pos, float* obst_vel,
                     int32_t* step, float* obs, float* reward, float* indiv_reward, uint8_t* done,
                     void* stream);

/* K consecutive fg_step_scenario calls in ONE launch (the landmark scenarios' counterpart of fg_rollout_hd; basic_formation_env
 * with scenario->kind = FG_SCN_BASIC): the state stays on chip, results are bit-identical to K single-step launches with
 * rng_offset, rng_offset + 1, ... (params->auto_reset included).  act_seq float [K][B][N][2]; reward_seq, indiv_seq float
 * [K][B][N]; done_seq uint8 [K][B][N]; near_ag_seq int32 [K][B][L] (basic only, may be NULL); obs_seq float
 * [K / obs_every][B][N][D] (steps k with (k+1) % obs_every == 0).  K = 0 is a no-op. */
int fg_rollout_scenario(const FgParams* params, const FgScenario* scenario, int B, int N, int K,
                        float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                        const float* act_seq, float* landmarks, float* obst_pos, float* obst_vel,
                        int32_t* step, float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq,
                        int32_t* near_ag_seq, int obs_every, void* stream);

/* Scenario.reset_world of the landmark scenarios on device for the envs whose mask byte is non-zero (mask NULL = all),
 * counter-based RNG (basic_formation_env.py:54-65, formation_hd_partial_env.py:88-99, formation_hd_partial_range_env.py:76-87,
 * formation_hd_obs_env.py:101-114 draw distribution): agent and landmark positions ~ U(-1,1)^2, velocities 0, obstacle k
 * ~ U([s_k, 2.0], [s_k+1, 2.5]) with s = linspace(-1.8, 1.8, M + 1) and velocity (obstacle_vx, obstacle_vy), step = 0.
 * basic_formation_env: scenario->kind = FG_SCN_BASIC, num_landmarks = L, num_obstacles = 0. */
int fg_reset_scenario(const FgParams* params, const FgScenario* scenario, int B, int N, const uint8_t* mask,
                      float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                      float* landmarks, float* obst_pos, float* obst_vel, int32_t* step, void* stream);

/* Action decoding of MultiAgentEnv._set_action (environment.py:187-215) for the non-default action
 * modes, before the sensitivity scaling (which the step kernels apply).  `count` = B*N agents.
 *   FG_ACT_ONEHOT5 (discrete_action_space, :207-210): action float [count][5] -> u = (a1 - a2, a3 - a4)
 *   FG_ACT_INDEX   (discrete_action_input, :194-205): action int32 [count], 1:-x 2:+x 3:-y 4:+y, else 0
 *   FG_ACT_ARGMAX  (force_discrete_action, :212-216): action float [count][2] -> one-hot of the arg-max
 *                   (first maximum, as np.argmax); the one-hot is also written back to `action`,
 *                   as the reference overwrites the caller's array
 * u_out float [count][2] is what fg_step_hd & co. take as `act`. */
#define FG_ACT_ONEHOT5 1
#define FG_ACT_INDEX 2
#define FG_ACT_ARGMAX 3
int fg_decode_actions(int mode, int64_t count, void* action, float* u_out, void* stream);

/* The reference's built-in demo controller for formation_hd_env, all B envs in one launch:
 * formation_gym.get_action_BFS(formation_gym.ezpolicy, obs_n, per_layer) (formation_gym/__init__.py:49-99
 * driving :19-47; caller test.py:23).  N must be per_layer^L with 2 <= per_layer <= 8.
 *   obs  float [B][N][6N] as fg_step_hd / fg_observe_hd write it (only row 0 of every env is read: relative
 *        positions, ideal shape, ideal velocity); obs_env_stride = floats between consecutive envs, 0 = 6 N^2
 *   act  float [B][N][2] raw actions, what fg_step_hd takes as `act`. */
int fg_policy_bfs(int B, int N, int per_layer, const float* obs, int64_t obs_env_stride, float* act, void* stream);

/* The same controller evaluated straight from the simulator state (no observation buffer needed); bit-identical
 * to fg_policy_bfs on the observation fg_observe_hd / fg_step_hd writes for that state. */
int fg_policy_bfs_state(int B, int N, int per_layer, const float* pos_x, const float* pos_y,
                        const float* ideal_shape, const float* ideal_vel, float* act, void* stream);

/* Closed-loop rollout with the built-in controller: the loop of test.py:17-27
 *     act_n = get_action_BFS(ezpolicy, obs_n, per_layer); obs_n, ... = env.step(act_n)
 * for K steps and all B envs.  Like fg_rollout_hd, except that act_seq [K][B][N][2] is an OUTPUT (the actions
 * taken, required).  For N in {3, 9, 27, 81, 243} with per_layer = 3 the controller runs inside the pipelined
 * rollout kernels (ONE launch); otherwise K x (controller launch + step launch) are chained on `stream`.
 * Results equal K x (fg_policy_bfs on the last observation, fg_step_hd) bit for bit. */
int fg_rollout_hd_policy(const FgParams* params, int B, int N, int K, int per_layer,
                         float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                         float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                         float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq,
                         int obs_every, void* stream);

/* 16-bit observations out of the rollout launch itself.  obs_format: */
#define FG_OBS_F16 1     /* IEEE binary16 (torch.float16) */
#define FG_OBS_BF16 2    /* bfloat16 */
/* fg_rollout_hd with obs_seq [K / obs_every][B][N][6N] in `obs_format` (2 bytes per element; 16-byte aligned, required,
 * contiguous): every element is the round-to-nearest-even conversion of the fp32 value fg_rollout_hd stores there - what a
 * second pass `obs.to(dtype)` over the fp32 tensor gives, bit for bit (fp16: overflow to inf, subnormals kept; signed zeros
 * kept) - written by the rollout kernel's writer waves as 16-byte stores, so that the launch moves half the observation bytes
 * and the caller's cast pass (read 4 B, write 2 B per element) goes away.  Everything else - state, reward_seq, indiv_seq,
 * done_seq, the RNG counter - is fg_rollout_hd's, bit for bit.
 * Fused support: formation_hd_env at N in {3, 9, 27} (the reference's hierarchy counts rollout_kernel serves), K >= 2.
 * Status: FG_ERR_UNSUPPORTED_N for any other N; FG_ERR_BAD_ARG for an unknown obs_format, K < 2, a padded env pitch
 * (params->obs_env_pitch != 0) or anything fg_rollout_hd would not run in the pipelined rollout kernel (walls, u_noise,
 * max_speed, accel, agent_props, comm_state); FG_ERR_ALIGNMENT for an obs_seq that is not 16-byte aligned.  There is no
 * fall-back inside the library: a caller that gets one of these runs fg_rollout_hd and casts.  B == 0 returns FG_OK without
 * a launch. */
int fg_rollout_hd_obs16(const FgParams* params, int obs_format, int B, int N, int K,
                        float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                        const float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                        void* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq,
                        int obs_every, void* stream);
/* ... and fg_rollout_hd_policy likewise (act_seq is an OUTPUT); per_layer must be 3 (else FG_ERR_UNSUPPORTED_N). */
int fg_rollout_hd_policy_obs16(const FgParams* params, int obs_format, int B, int N, int K, int per_layer,
                               float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                               float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                               void* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq,
                               int obs_every, void* stream);
/* Dry run of fg_rollout_hd_obs16 (per_layer = 0) or fg_rollout_hd_policy_obs16 (per_layer = 3): the same checks and status
 * codes (those on the buffers apart; B > 0 required), then "rollout_kernel<NC,G,TP,TW,E,WR,PER,STREAM> grid G lds L; " in
 * `out` as fg_describe_launch writes it, WR being the 16-bit writer of the format (65: fp16, 66: bf16).  Touches no device:
 * this is how a caller decides between the fused launch and fg_rollout_hd + cast. */
int fg_describe_obs16_launch(const FgParams* params, int obs_format, int B, int N, int K, int per_layer, int obs_every,
                             char* out, int out_len);

/* The caller's MLP actor for fg_rollout_hd_actor: Linear(6N, hidden) - ReLU - Linear(hidden, hidden) - ReLU -
 * Linear(hidden, 2) [- tanh], one actor shared by every agent.  Weights in the torch Linear layout [out][in], fp32, in
 * DEVICE memory, read in place by every launch (an optimizer step between two launches is seen by the next one); a NULL
 * bias counts as zero.  hidden: 32, 64 or 128. */
typedef struct FgActor {
    int32_t hidden;
    int32_t out_tanh;        /* 1: tanh on the two outputs */
    const float* w1;         /* [hidden][6N] */
    const float* b1;         /* [hidden] or NULL */
    const float* w2;         /* [hidden][hidden] */
    const float* b2;         /* [hidden] or NULL */
    const float* w3;         /* [2][hidden] */
    const float* b3;         /* [2] or NULL */
} FgActor;

/* Closed-loop rollout with the caller's actor: the loop of a learned policy
 *     act_n = actor(obs_n); obs_n, ... = env.step(act_n)
 * for K >= 1 steps and all B envs of formation_hd_env, in ONE launch (actor_rollout_kernel): step 0 acts on the
 * observation of the current state, step k on the observation step k-1 returned (after the device auto-reset, when
 * params->auto_reset is set).  Arguments as fg_rollout_hd_policy's - act_seq [K][B][N][2] is an OUTPUT (the actions taken,
 * required), obs_env_pitch, obs_placed, auto-reset and rng_offset / rng_offset_dev as documented above - and the results
 * equal fg_rollout_hd driven by the recorded act_seq bit for bit.  N in {3, 4, 8, 9, 16, 25, 27, 32}, silent agents and no
 * World options (walls, accel, max_speed, u_noise, agent_props, comm_state): anything else returns FG_ERR_UNSUPPORTED_N
 * (N) or FG_ERR_BAD_ARG; there is no fall-back inside the library. */
int fg_rollout_hd_actor(const FgParams* params, const FgActor* actor, int B, int N, int K,
                        float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                        float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                        float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq,
                        int obs_every, void* stream);
/* Dry run of fg_rollout_hd_actor: the kernel instantiation and launch geometry it would use, written to `out` as text,
 * after the same checks (same status codes).  Touches no device. */
int fg_describe_actor_launch(const FgParams* params, const FgActor* actor, int B, int N, int K, int obs_every,
                             char* out, int out_len);

/* fg_rollout_hd_actor with a diagonal Gaussian on top of the actor (actor_sample_kernel): step k takes
 *     a = actor(o) + exp(log_std) * eps,    log_prob = -(eps_0^2 + eps_1^2) / 2 - (log_std_0 + log_std_1) - log(2 pi)
 * where log_std [2] is fp32 in DEVICE memory, state-independent and read in place by every launch, and eps [2] of agent i of
 * env b is fg_actor_noise's draw at step k's counter offset (rng_base + k, the offset of step k's auto-reset): Philox4x32-10
 * keyed by params->seed on the counter {b + env_index_base, i ^ 0xA0000000, lo32(offset), hi32(offset)}, then Box-Muller on
 * words 0 and 1.  No clipping, no tanh after the noise.  logp_seq [K][B][N] receives log_prob (NULL: not written); every
 * other argument, check and status code is fg_rollout_hd_actor's.  A NULL log_std returns FG_ERR_BAD_ARG. */
int fg_rollout_hd_actor_sample(const FgParams* params, const FgActor* actor, const float* log_std, int B, int N, int K,
                               float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                               float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                               float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                               int obs_every, void* stream);
/* One step's exploration noise of fg_rollout_hd_actor_sample: eps [B][N][2] (8-byte aligned, device memory) at the counter
 * offset rng_base(params) (rng_offset + *rng_offset_dev), from the same device function as the fused kernel - the
 * host-paced loop of a Gaussian actor calls it once per step and draws the same numbers.  `params` passes the usual checks;
 * the draw reads only its seed, env_index_base and offset.  N < 2^29 (the stream's counter word keeps three top bits). */
int fg_actor_noise(const FgParams* params, int B, int N, float* eps, void* stream);
/* The log-density of `count` draws: logp [count] = -(eps_0^2 + eps_1^2) / 2 - (log_std_0 + log_std_1) - log(2 pi) for
 * eps [count][2] (8-byte aligned) and log_std [2], all fp32 in DEVICE memory, from the device function the fused Gaussian
 * kernels use (the same bits as their logp_seq for the same eps and log_std): the host-paced loop of a Gaussian actor calls
 * it once per step on fg_actor_noise's draw.  count == 0 is a no-op. */
int fg_actor_log_prob(const float* eps, const float* log_std, int64_t count, float* logp, void* stream);
/* Dry run of fg_rollout_hd_actor_sample (the twin of fg_describe_actor_launch): same checks and status codes, names the
 * actor_sample_kernel<N,H> instantiation.  Touches no device; log_std is only checked for NULL and alignment. */
int fg_describe_actor_sample_launch(const FgParams* params, const FgActor* actor, const float* log_std, int B, int N, int K,
                                    int obs_every, char* out, int out_len);

/* fg_rollout_hd_actor / fg_rollout_hd_actor_sample with one actor per agent (MADDPG-style, no parameter sharing): `actors`
 * is a HOST array of N FgActor, agent i's observation rows go through actors[i] (pa_actor_kernel, or pa_sample_kernel when
 * log_std is not NULL).  Every member passes fg_rollout_hd_actor's checks and has the hidden width and tanh flag of
 * actors[0] (else FG_ERR_BAD_ARG, the message names the member's index); the table of pointers is copied into the launch,
 * so `actors` may be freed when the call returns, while the weights it points at are read in place by the kernel.
 * log_std == NULL: the deterministic actor, logp_seq ignored; else log_std [2] and logp_seq as in fg_rollout_hd_actor_sample
 * (the same eps draws).  N identical members give the results of fg_rollout_hd_actor(_sample) with that member bit for bit. */
int fg_rollout_hd_actor_per_agent(const FgParams* params, const FgActor* actors, const float* log_std, int B, int N, int K,
                                  float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                                  float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                                  float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                                  int obs_every, void* stream);
/* Dry run of fg_rollout_hd_actor_per_agent: same checks and status codes, names the pa_actor_kernel<N,H> or
 * pa_sample_kernel<N,H> instantiation.  Touches no device. */
int fg_describe_actor_per_agent_launch(const FgParams* params, const FgActor* actors, const float* log_std, int B, int N,
                                       int K, int obs_every, char* out, int out_len);

/* The LayerNorms of fg_rollout_hd_actor_norm's actor (the MAPPO trainers' actor, onpolicy's MLPBase):
 *     [LayerNorm(6N) -] Linear(6N, hidden) - ReLU - LayerNorm(hidden) - Linear(hidden, hidden) - ReLU - LayerNorm(hidden) -
 *     Linear(hidden, 2) [- tanh]
 * in_*: the norm over the actor's input, present when in_norm is 1 (else in_gamma, in_beta and in_eps are not read);
 * h1_*, h2_*: the norms after the first and the second ReLU.  gamma / beta: fp32 [width] in DEVICE memory, read in place by
 * every launch like the weights; NULL is the identity (gamma 1, beta 0).  Each norm is torch.nn.LayerNorm over the last axis:
 * mean and biased variance of the row in fp32 (the variance from the centred values), y = (x - mean) / sqrt(var + eps) *
 * gamma + beta, with its own positive, finite eps. */
typedef struct FgActorNorm {
    const float* in_gamma;   /* [6N] or NULL */
    const float* in_beta;    /* [6N] or NULL */
    const float* h1_gamma;   /* [hidden] or NULL */
    const float* h1_beta;    /* [hidden] or NULL */
    const float* h2_gamma;   /* [hidden] or NULL */
    const float* h2_beta;    /* [hidden] or NULL */
    float in_eps;
    float h1_eps;
    float h2_eps;
    int32_t in_norm;         /* 1: the actor starts with a LayerNorm over its input */
} FgActorNorm;

/* fg_rollout_hd_actor (log_std == NULL; logp_seq ignored) or fg_rollout_hd_actor_sample (log_std [2] and logp_seq as there,
 * the same eps draws) with the LayerNorm actor `actor` + `norm` shared by every agent (ln_actor_kernel / ln_sample_kernel).
 * actor->hidden: 32 or 64.  Every other argument, check and status code is fg_rollout_hd_actor_sample's
 * (FG_ERR_UNSUPPORTED_N for N as in fg_rollout_hd_actor); FG_ERR_BAD_ARG, the message naming the field, for a NULL norm, an
 * eps that is not positive and finite, a gamma / beta pointer that is not 4-byte aligned, or hidden = 128.  Two launches from
 * one state give the same bits, and fg_rollout_hd driven by the recorded act_seq returns the same results bit for bit. */
int fg_rollout_hd_actor_norm(const FgParams* params, const FgActor* actor, const FgActorNorm* norm, const float* log_std,
                             int B, int N, int K, float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                             float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                             float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                             int obs_every, void* stream);
/* Dry run of fg_rollout_hd_actor_norm: same checks and status codes, names the ln_actor_kernel<N,H> or
 * ln_sample_kernel<N,H> instantiation and its launch geometry.  Touches no device. */
int fg_describe_actor_norm_launch(const FgParams* params, const FgActor* actor, const FgActorNorm* norm, const float* log_std,
                                  int B, int N, int K, int obs_every, char* out, int out_len);

/* The recurrent layer of fg_rollout_hd_actor_gru's actor (rMAPPO's policy: onpolicy's R_Actor with use_recurrent_policy and
 * recurrent_N = 1), between the LayerNorm body and the action head:
 *     [LayerNorm(6N) -] Linear(6N, hidden) - ReLU - LayerNorm(hidden) - Linear(hidden, hidden) - ReLU - LayerNorm(hidden) -
 *     GRU(hidden, hidden) - LayerNorm(hidden) - Linear(hidden, 2) [- tanh]
 * One step of torch.nn.GRUCell / a single-layer unidirectional torch.nn.GRU per actor evaluation, gate order r | z | n:
 *     r = sigmoid(W_ir x + b_ir + W_hr h + b_hr),  z = sigmoid(W_iz x + b_iz + W_hz h + b_hz),
 *     n = tanh(W_in x + b_in + r * (W_hn h + b_hn)),  h' = (1 - z) * n + z * h
 * h' is the state carried to the next step; the head sees LayerNorm(h').  All tensors fp32 in DEVICE memory, torch's layout
 * (weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0), read in place by every launch; the four of them are required.
 * norm_gamma / norm_beta: the LayerNorm after the GRU, NULL is the identity (gamma 1, beta 0); norm_eps positive and finite. */
typedef struct FgActorGru {
    const float* w_ih;       /* [3 hidden][hidden] */
    const float* w_hh;       /* [3 hidden][hidden] */
    const float* b_ih;       /* [3 hidden] */
    const float* b_hh;       /* [3 hidden] */
    const float* norm_gamma; /* [hidden] or NULL */
    const float* norm_beta;  /* [hidden] or NULL */
    float norm_eps;
} FgActorGru;

/* fg_rollout_hd_actor_norm with the recurrent layer `gru` between the body and its last Linear (gru_actor_kernel, or
 * gru_sample_kernel when log_std is not NULL): `actor` and `norm` describe the body, actor->w3 / b3 the head on
 * LayerNorm(h').  The loop of the launch, for k = 0 .. K - 1:
 *     a, h = actor(obs, h);  obs, ..., done = env.step(a);  h = 0 in every env whose step k ended its episode
 * (the step's own done flag, whether or not params->auto_reset is set).  rnn_state [B][N][hidden], fp32, 16-byte aligned, is
 * the state step 0 acts with and receives the state after step K - 1, already masked; in between it lives on chip.  A K-step
 * call equals K one-step calls that pass the state along, bit for bit.  actor->hidden: 32 or 64.  Every other argument,
 * check and status code is fg_rollout_hd_actor_norm's, in this entry's name; then FG_ERR_BAD_ARG, the message naming the
 * field, for a NULL gru, a NULL w_ih / w_hh / b_ih / b_hh, a NULL rnn_state with B > 0, or a norm_eps that is not positive
 * and finite, and FG_ERR_ALIGNMENT for a gru pointer that is not 4-byte or an rnn_state that is not 16-byte aligned. */
int fg_rollout_hd_actor_gru(const FgParams* params, const FgActor* actor, const FgActorNorm* norm, const FgActorGru* gru,
                            const float* log_std, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                            float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                            float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                            float* rnn_state, int obs_every, void* stream);
/* fg_rollout_hd_actor_gru that also keeps the hidden states a recurrent PPO update restarts from (onpolicy's
 * rnn_states[step]): rnn_states [ceil(K / states_every)][B][N][hidden], fp32, 16-byte aligned, an OUTPUT.  Entry j is the state
 * step j * states_every ACTED WITH: entry 0 is rnn_state as passed in, entry j > 0 is already zero in every env whose step
 * j * states_every - 1 ended its episode.  states_every = 1 keeps every step's state, states_every = the update's chunk length
 * only what its chunks start from, states_every > K entry 0 alone.  Nothing else of the launch changes: the same kernel and
 * geometry (fg_describe_actor_gru_launch), the same bits in every other output and in rnn_state.  Every other argument, check
 * and status code is fg_rollout_hd_actor_gru's, in this entry's name; then FG_ERR_BAD_ARG for states_every < 1 or a NULL
 * rnn_states with B > 0, and FG_ERR_ALIGNMENT for an rnn_states that is not 16-byte aligned.  B == 0 returns FG_OK. */
int fg_rollout_hd_actor_gru_states(const FgParams* params, const FgActor* actor, const FgActorNorm* norm, const FgActorGru* gru,
                                   const float* log_std, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x,
                                   float* vel_y, float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                                   float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                                   float* rnn_state, float* rnn_states, int states_every, int obs_every, void* stream);
/* Dry run of fg_rollout_hd_actor_gru: same checks and status codes (rnn_state's apart), names the gru_actor_kernel<N,H> or
 * gru_sample_kernel<N,H> instantiation and its launch geometry.  Touches no device. */
int fg_describe_actor_gru_launch(const FgParams* params, const FgActor* actor, const FgActorNorm* norm, const FgActorGru* gru,
                                 const float* log_std, int B, int N, int K, int obs_every, char* out, int out_len);

/* The eval-mode input BatchNorm of fg_rollout_hd_actor_bn's actor (the MADDPG trainers' MLPNetwork with norm_in: `in_fn`, one
 * network per agent, `policy.eval()` while acting):
 *     BatchNorm1d(6N) - Linear(6N, hidden) - ReLU - Linear(hidden, hidden) - ReLU - Linear(hidden, 2) [- tanh]
 * torch.nn.BatchNorm1d on its running statistics, per feature k:
 *     y_k = (x_k - mean_k) / sqrt(var_k + eps) * gamma_k + beta_k
 * All tensors fp32 [6N] in DEVICE memory, read in place by every launch like the weights (a changed statistic is seen by the
 * next launch).  Batch statistics (training mode) are a function of the whole batch and have no fused launch.  Out of scope:
 * hidden = 128, a BatchNorm anywhere but first or with the LayerNorm / GRU bodies, and the landmark scenarios.  MADDPG's
 * exploration on top of it - OU noise and the clamp after it - is fg_rollout_hd_actor_ou's; fg_rollout_hd_actor_sample's Gaussian
 * noise stays unclipped. */
typedef struct FgActorInBn {
    const float* mean;    /* [6N] running mean */
    const float* var;     /* [6N] running variance */
    const float* gamma;   /* [6N] or NULL: 1 */
    const float* beta;    /* [6N] or NULL: 0 */
    float eps;            /* positive, finite */
} FgActorInBn;

/* fg_rollout_hd_actor (log_std == NULL; logp_seq ignored) or fg_rollout_hd_actor_sample (log_std [2] and logp_seq as there, the
 * same eps draws) with the actor `actor` behind the input BatchNorm `in_bn`, shared by every agent (bn_actor_kernel /
 * bn_sample_kernel).  actor->hidden: 32 or 64.  Every other argument, check and status code is fg_rollout_hd_actor_sample's; then
 * FG_ERR_BAD_ARG, the message naming the field, for a NULL in_bn, a NULL mean or var, an eps that is not positive and finite,
 * or hidden = 128, and FG_ERR_ALIGNMENT for a mean, var, gamma or beta that is not 4-byte aligned.  Two launches from one
 * state give the same bits, and fg_rollout_hd driven by the recorded act_seq returns the same results bit for bit. */
int fg_rollout_hd_actor_bn(const FgParams* params, const FgActor* actor, const FgActorInBn* in_bn, const float* log_std,
                           int B, int N, int K, float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                           float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                           float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                           int obs_every, void* stream);
/* fg_rollout_hd_actor_per_agent with member i's network behind its own input BatchNorm in_bns[i] (pa_bn_actor_kernel /
 * pa_bn_sample_kernel): `actors` and `in_bns` are HOST arrays of N entries, the tables of pointers and the eps values are copied
 * into the launch (both may be freed when the call returns), the tensors are read in place.  Every check of
 * fg_rollout_hd_actor_per_agent, then fg_rollout_hd_actor_bn's for every member, the message naming the member's index.
 * N identical members give the results of fg_rollout_hd_actor_bn with that member bit for bit. */
int fg_rollout_hd_actor_bn_per_agent(const FgParams* params, const FgActor* actors, const FgActorInBn* in_bns,
                                     const float* log_std, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x,
                                     float* vel_y, float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                                     float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                                     int obs_every, void* stream);
/* Dry runs of the two: same checks and status codes, name the bn_actor_kernel<N,H> / bn_sample_kernel<N,H> or
 * pa_bn_actor_kernel<N,H> / pa_bn_sample_kernel<N,H> instantiation and its launch geometry.  Touch no device. */
int fg_describe_actor_bn_launch(const FgParams* params, const FgActor* actor, const FgActorInBn* in_bn, const float* log_std,
                                int B, int N, int K, int obs_every, char* out, int out_len);
int fg_describe_actor_bn_per_agent_launch(const FgParams* params, const FgActor* actors, const FgActorInBn* in_bns,
                                          const float* log_std, int B, int N, int K, int obs_every, char* out, int out_len);

/* MADDPG's exploration on top of a deterministic actor (train/maddpg-v2: OUNoise, `scale`, the clamp after it).  Per
 * (env, agent) a noise state x [2] is carried from step to step; the step that takes an action does, per component,
 *     x <- x + theta (mu - x) + sigma eps          evaluated fma(sigma, eps, fma(theta, mu - x, x))
 *     a  = clamp(actor(o) + scale x, -clip, clip)  a product, a sum, max, min - torch's fp32 bits; clip = +inf: no clamp
 * with eps fg_actor_noise's draw at the step's counter offset (the draws of fg_rollout_hd_actor_sample: the same on either path
 * and under any sharding), and after a step whose done flag is set for the env - with or without auto_reset - x <- mu
 * (reset_noise(); the convention of fg_rollout_hd_actor_gru's state).  theta = 1, mu = 0 is the memoryless special case,
 * x = sigma eps: maddpg-v1's Gaussian noise and clip.  There is no log_std and no log-density. */
typedef struct FgActorOu {
    float theta;   /* in [0, 1] */
    float mu;      /* finite */
    float sigma;   /* finite, >= 0 */
    float scale;   /* finite */
    float clip;    /* > 0; +inf: no clamp */
} FgActorOu;

/* fg_rollout_hd_actor (in_bn == NULL) or fg_rollout_hd_actor_bn (in_bn: the input BatchNorm) with the exploration `ou` on the
 * actor's output (ou_actor_kernel / bn_ou_actor_kernel), hidden as there.  noise_state [B][N][2], fp32 in DEVICE memory, 8-byte
 * aligned: read as the state step 0 starts from, kept on chip for the launch, written back as the state after step K - 1
 * (already mu where that step ended an episode).  act_seq receives the clamped actions.  Every other argument, check and
 * status code is the inner entry's; then FG_ERR_BAD_ARG, the message naming the field, for a NULL ou, a theta outside [0, 1],
 * a negative sigma, a theta / mu / sigma / scale that is not finite, a clip that is NaN or not positive, a NULL noise_state
 * with B > 0, and FG_ERR_ALIGNMENT for a noise_state that is not 8-byte aligned.  B == 0 returns FG_OK.  A K-step launch equals
 * K one-step launches that pass noise_state along, bit for bit; two launches from one state give the same bits, and
 * fg_rollout_hd driven by the recorded act_seq returns the same results bit for bit. */
int fg_rollout_hd_actor_ou(const FgParams* params, const FgActor* actor, const FgActorInBn* in_bn, const FgActorOu* ou,
                           float* noise_state, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                           float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                           float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, int obs_every, void* stream);
/* ... with one actor per agent: fg_rollout_hd_actor_per_agent (in_bns == NULL) or fg_rollout_hd_actor_bn_per_agent (in_bns: a
 * HOST array of N) under the one `ou` (pa_ou_actor_kernel / pa_bn_ou_actor_kernel). */
int fg_rollout_hd_actor_ou_per_agent(const FgParams* params, const FgActor* actors, const FgActorInBn* in_bns, const FgActorOu* ou,
                                     float* noise_state, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x,
                                     float* vel_y, float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                                     float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, int obs_every,
                                     void* stream);
/* Dry runs of the two: same checks and status codes (noise_state's apart), name the ou_actor_kernel<N,H> / bn_ou_actor_kernel<N,H>
 * or pa_ou_actor_kernel<N,H> / pa_bn_ou_actor_kernel<N,H> instantiation and its launch geometry.  Touch no device. */
int fg_describe_actor_ou_launch(const FgParams* params, const FgActor* actor, const FgActorInBn* in_bn, const FgActorOu* ou,
                                int B, int N, int K, int obs_every, char* out, int out_len);
int fg_describe_actor_ou_per_agent_launch(const FgParams* params, const FgActor* actors, const FgActorInBn* in_bns,
                                          const FgActorOu* ou, int B, int N, int K, int obs_every, char* out, int out_len);
/* The state update alone, x <- x + theta (mu - x) + sigma eps, on `count` (env, agent) pairs in place - eps and state
 * [count][2], fp32 in DEVICE memory, 8-byte aligned - by the device function the fused kernels use: the host-paced loop calls
 * it once per step on fg_actor_noise's draw and carries the fused launch's state bits.  ou's checks as above; count == 0 is a
 * no-op. */
int fg_actor_ou_step(const FgActorOu* ou, int64_t count, const float* eps, float* state, void* stream);

/* The MAPPO trainers' discrete-action policy (make_env(..., discrete_action=True): a head Linear(hidden, 5) under a
 * Categorical) as the categorical member of the plain, LayerNorm and recurrent families: cat_actor_kernel (norm == NULL),
 * ln_cat_actor_kernel (norm) and gru_cat_actor_kernel (norm and gru), at those families' N and hidden widths.  The actor is
 * fg_rollout_hd_actor's / _norm's / _gru's with w3 [5][hidden], b3 [5] (or NULL) and out_tanh == 0.  Per (env b, agent i,
 * step k) the five fp32 logits l_j are ascending fmaf chains from b3[j], and, in fp32,
 *     m = max_j l_j,  e_j = exp(l_j - m),  c_j = e_0 + .. + e_j,  s = c_4          (exp: __expf, log below: __logf)
 *     sampled (greedy == 0): t = u s, idx the first j in 0..3 with t < c_j, else 4
 *     greedy  (greedy != 0): idx the lowest index attaining m (the distribution's mode)
 *     log_prob = (l_idx - m) - log(s)
 * with u = (c[2] >> 8) 2^-24 in [0, 1), c the Philox4x32-10 block fg_actor_noise draws for (b, i, k) - key seed, counter
 * {b + env_index_base, i ^ 0xA0000000, lo32(off), hi32(off)}, off = rng_base + k; its words 0 and 1 stay the Gaussian members'
 * draw.  The index becomes the raw action u by act_mode, the env's own: FG_ACT_ONEHOT5 takes the one-hot e_idx through
 * (a1 - a2, a3 - a4) - 1: +x, 2: -x, 3: +y, 4: -y - and FG_ACT_INDEX is fg_decode_actions' 1: -x, 2: +x, 3: -y, 4: +y; index 0
 * is no move.  `greedy` and `act_mode` are run-time facts of the launch: one kernel per (family, N, hidden).
 * act_seq [K][B][N][2] (required) receives the decoded u, so fg_rollout_hd driven by it returns the same results bit for bit;
 * idx_seq [K][B][N] int32 (required) the indices, logp_seq [K][B][N] (NULL: not written) the log-probs.  rnn_state [B][N][hidden]
 * (gru only; else ignored) as in fg_rollout_hd_actor_gru; rnn_states (NULL: none kept) / states_every as in
 * fg_rollout_hd_actor_gru_states.  Checks and status codes are fg_rollout_hd_actor_norm's / _gru's in their order; in addition
 * FG_ERR_BAD_ARG for out_tanh != 0, an act_mode other than the two above (FG_ACT_ARGMAX included), gru without norm, a NULL
 * idx_seq with B > 0, and FG_ERR_ALIGNMENT for an idx_seq or logp_seq that is not 4-byte aligned.  B == 0 returns FG_OK. */
int fg_rollout_hd_actor_cat(const FgParams* params, const FgActor* actor, const FgActorNorm* norm, const FgActorGru* gru,
                            int act_mode, int greedy, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                            float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                            float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, int32_t* idx_seq,
                            float* logp_seq, float* rnn_state, float* rnn_states, int states_every, int obs_every, void* stream);
/* Dry run: same checks and status codes (the buffers' apart), names the cat_actor_kernel<N,H> / ln_cat_actor_kernel<N,H> /
 * gru_cat_actor_kernel<N,H> instantiation and its launch geometry.  Touches no device. */
int fg_describe_actor_cat_launch(const FgParams* params, const FgActor* actor, const FgActorNorm* norm, const FgActorGru* gru,
                                 int act_mode, int greedy, int B, int N, int K, int obs_every, char* out, int out_len);

/* 16-bit observations out of the fused actor launch: the Gaussian member of the plain (norm == NULL), LayerNorm (norm) and
 * recurrent (norm and gru) family - fg_rollout_hd_actor_sample / _norm / _gru_states with a log_std, which is required - with
 * obs_seq [K / obs_every][B][N][6N] in `obs_format` (FG_OBS_F16 / FG_OBS_BF16; 2 bytes per element, 16-byte aligned, contiguous;
 * NULL: not written).  Every element is the round-to-nearest-even conversion of the fp32 value the fp32 entry stores there -
 * what `obs.to(dtype)` gives, bit for bit (fp16: overflow to inf, subnormals kept; signed zeros kept) - stored by the kernel's
 * stream phase through the 16-bit tile writer of fg_rollout_hd_obs16 (wave-private LDS tiles in the wave's activation tile, 16
 * bytes per lane and store).  Everything else - act_seq, logp_seq, reward_seq, indiv_seq, done_seq, rnn_state, rnn_states, the
 * state and the RNG counter - is the fp32 entry's, bit for bit.  The format is a run-time fact of the launch: one kernel
 * (actor_sample_obs16 / ln_sample_obs16 / gru_sample_obs16 <N,H>) serves both.  rnn_state (gru only; else ignored), rnn_states
 * (NULL: none kept) and states_every as in fg_rollout_hd_actor_gru_states; K >= 1, any obs_every.
 * Fused support: N in {3, 9, 27}, hidden in {32, 64}, no World options.  Status, checked in this order and in this entry's
 * name: FG_ERR_BAD_ARG for an unknown obs_format, a padded env pitch (params->obs_env_pitch != 0) or a NULL log_std;
 * FG_ERR_UNSUPPORTED_N for any other N; FG_ERR_BAD_ARG for hidden = 128; then every check of the fp32 entries in their order
 * (FG_ERR_ALIGNMENT for an obs_seq that is not 16-byte aligned among the buffers').  There is no fall-back inside the library:
 * a caller that gets one of these runs the fp32 entry and casts.  B == 0 returns FG_OK without a launch. */
int fg_rollout_hd_actor_obs16(const FgParams* params, int obs_format, const FgActor* actor, const FgActorNorm* norm,
                              const FgActorGru* gru, const float* log_std, int B, int N, int K, float* pos_x, float* pos_y,
                              float* vel_x, float* vel_y, float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                              void* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                              float* rnn_state, float* rnn_states, int states_every, int obs_every, void* stream);
/* ... and the categorical member likewise: fg_rollout_hd_actor_cat's arguments and checks behind the same first ones (there is
 * no log_std), kernels cat_actor_obs16 / ln_cat_actor_obs16 / gru_cat_actor_obs16 <N,H>. */
int fg_rollout_hd_actor_cat_obs16(const FgParams* params, int obs_format, const FgActor* actor, const FgActorNorm* norm,
                                  const FgActorGru* gru, int act_mode, int greedy, int B, int N, int K, float* pos_x, float* pos_y,
                                  float* vel_x, float* vel_y, float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                                  void* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, int32_t* idx_seq,
                                  float* logp_seq, float* rnn_state, float* rnn_states, int states_every, int obs_every,
                                  void* stream);
/* Dry runs: the same checks and status codes (the buffers' apart; B > 0 required), then the instantiation, grid and LDS as
 * fg_describe_actor_launch writes them; the name does not depend on the format.  Touch no device: this is how a caller
 * decides between the fused 16-bit launch and the fp32 entry + cast. */
int fg_describe_actor_obs16_launch(const FgParams* params, int obs_format, const FgActor* actor, const FgActorNorm* norm,
                                   const FgActorGru* gru, const float* log_std, int B, int N, int K, int obs_every, char* out,
                                   int out_len);
int fg_describe_actor_cat_obs16_launch(const FgParams* params, int obs_format, const FgActor* actor, const FgActorNorm* norm,
                                       const FgActorGru* gru, int act_mode, int greedy, int B, int N, int K, int obs_every,
                                       char* out, int out_len);
/* One step's uniform draws u [B][N] (fp32 in DEVICE memory, 4-byte aligned) at rng_base(params), by the device function of
 * the categorical kernels: fg_actor_noise's sibling for the host-paced loop of a categorical policy. */
int fg_actor_uniform(const FgParams* params, int B, int N, float* u, void* stream);
/* The pick above and the decode on `count` rows of caller-supplied logits [count][5] and draws u [count] (NULL allowed when
 * greedy), by the fused kernels' device functions: idx [count] int32 (required), act [count][2] (8-byte aligned; NULL: not
 * written), logp [count] (NULL: not written), all fp32 / int32 in DEVICE memory.  The host-paced loop calls it once per step
 * on the module's logits and fg_actor_uniform's draw.  FG_ERR_BAD_ARG for another act_mode, a negative count, a NULL logits,
 * idx or (sampling) u; count == 0 is a no-op. */
int fg_actor_categorical(int act_mode, int greedy, int64_t count, const float* logits, const float* u, int32_t* idx, float* act,
                         float* logp, void* stream);

/* The MADDPG trainers' discrete actions (maddpg-pytorch's agents on make_env(..., discrete_action=True): exploring,
 * gumbel_softmax(logits, hard=True); otherwise onehot_from_logits(logits)) as the Gumbel member of the four families without
 * LayerNorms - the discrete twin of fg_rollout_hd_actor_ou: gumbel_actor_kernel (in_bn == NULL) or bn_gumbel_actor_kernel
 * (in_bn: the input BatchNorm), at those families' N and hidden widths (128 without, 64 with the BatchNorm).  The actor is
 * fg_rollout_hd_actor's / _bn's with w3 [5][hidden], b3 [5] (or NULL) and out_tanh == 0.  Per (env b, agent i, step k) the five
 * fp32 logits l_j are ascending fmaf chains from b3[j], as in fg_rollout_hd_actor_cat, and
 *     Gumbel draws: five per row from a Philox4x32-10 stream of their own - key seed, counter
 *         {b + env_index_base, i | 0x60000000 | (q << 12), lo32(off), hi32(off)}, off = rng_base + k;
 *         draw j is word j & 3 of block q = j >> 2 (block 0: j = 0..3, word 0 of block 1: j = 4).  The top three bits of word 1
 *         are 011 against 000 / 001 / 100 / 101 / 110 / 111 of every other stream, and the actor-noise block is not touched:
 *         Gaussian, OU and categorical draws keep their bits.
 *         u_j = (2 (c >> 9) + 1) 2^-24 - an odd 24-bit integer scaled: exact in fp32, strictly inside (0, 1) -
 *         g_j = -log(-log(u_j)) in [-2.82, 16.64], both logarithms the full-precision fp32 log (not the hardware approximation:
 *         the inner result is the outer logarithm's argument).
 *     exploring (explore != 0): y_j = l_j + g_j, one fp32 addition of the finished logit, never contracted into its chain
 *     otherwise (explore == 0): y_j = l_j, no draws
 *     idx = the lowest j attaining max_j y_j
 * gumbel_softmax's temperature does not enter - argmax softmax(y / T) = argmax y for every T > 0 - and its soft sample
 * (hard=False), a training-time quantity, is not built; nor is onehot_from_logits' epsilon-greedy.  The index becomes the raw
 * action by act_mode, the env's own, exactly as in fg_rollout_hd_actor_cat (FG_ACT_ONEHOT5, MADDPG's, or FG_ACT_INDEX).  There
 * is no log-prob.  `explore` and `act_mode` are run-time facts of the launch: one kernel per (family, N, hidden).
 * act_seq [K][B][N][2] (required) receives the decoded raw action, so fg_rollout_hd driven by it returns the same results bit
 * for bit; idx_seq [K][B][N] int32 (required) the indices.  Checks and status codes are the inner entry's (fg_rollout_hd_actor's
 * / _bn's) in their order, in this entry's name; then FG_ERR_BAD_ARG for out_tanh != 0, an act_mode other than the two
 * (FG_ACT_ARGMAX included), a NULL idx_seq with B > 0, and FG_ERR_ALIGNMENT for an idx_seq that is not 4-byte aligned.  B == 0
 * returns FG_OK.  Two launches from one state give the same bits. */
int fg_rollout_hd_actor_gumbel(const FgParams* params, const FgActor* actor, const FgActorInBn* in_bn, int act_mode,
                               int explore, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                               float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                               float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, int32_t* idx_seq,
                               int obs_every, void* stream);
/* ... with one actor per agent (MADDPG's one MLPNetwork per agent): fg_rollout_hd_actor_per_agent (in_bns == NULL) or
 * fg_rollout_hd_actor_bn_per_agent (in_bns: a HOST array of N), kernels pa_gumbel_actor_kernel / pa_bn_gumbel_actor_kernel.  N
 * identical members give the shared kernel's indices and actions bit for bit. */
int fg_rollout_hd_actor_gumbel_per_agent(const FgParams* params, const FgActor* actors, const FgActorInBn* in_bns, int act_mode,
                                         int explore, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x,
                                         float* vel_y, float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                                         float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, int32_t* idx_seq,
                                         int obs_every, void* stream);
/* Dry runs of the two: same checks and status codes (the buffers' apart), name the gumbel_actor_kernel<N,H> /
 * bn_gumbel_actor_kernel<N,H> or pa_gumbel_actor_kernel<N,H> / pa_bn_gumbel_actor_kernel<N,H> instantiation and its launch
 * geometry.  Touch no device. */
int fg_describe_actor_gumbel_launch(const FgParams* params, const FgActor* actor, const FgActorInBn* in_bn, int act_mode,
                                    int explore, int B, int N, int K, int obs_every, char* out, int out_len);
int fg_describe_actor_gumbel_per_agent_launch(const FgParams* params, const FgActor* actors, const FgActorInBn* in_bns,
                                              int act_mode, int explore, int B, int N, int K, int obs_every, char* out,
                                              int out_len);
/* One step's Gumbel draws g [B][N][5] (fp32 in DEVICE memory, 4-byte aligned) at rng_base(params), by the device function of
 * the Gumbel kernels: fg_actor_uniform's sibling for the host-paced loop of a Gumbel-softmax policy.  1 <= N <= 2^12. */
int fg_actor_gumbel(const FgParams* params, int B, int N, float* g, void* stream);
/* The pick above and the decode on `count` rows of caller-supplied logits [count][5] and draws g [count][5] (NULL allowed when
 * not exploring), by the fused kernels' device functions: idx [count] int32 (required), act [count][2] (8-byte aligned; NULL:
 * not written), all fp32 / int32 in DEVICE memory.  FG_ERR_BAD_ARG for another act_mode, a negative count, a NULL logits, idx or
 * (exploring) g; FG_ERR_ALIGNMENT for a misaligned buffer; count == 0 is a no-op. */
int fg_actor_gumbel_pick(int act_mode, int explore, int64_t count, const float* logits, const float* g,
                         int32_t* idx, float* act, void* stream);

/* fg_rollout_hd_actor / fg_rollout_hd_actor_sample for the landmark scenarios (basic_formation_env, formation_hd_partial_env,
 * formation_hd_partial_range_env, formation_hd_obs_env): K >= 1 closed-loop steps of all B envs in ONE launch
 * (scn_lane_actor, or scn_lane_actor_gauss when log_std is not NULL), with the actor
 *     Linear(D, hidden) - ReLU - Linear(hidden, hidden) - ReLU - Linear(hidden, 2) [- tanh],   hidden 32 or 64,
 * D the scenario's observation width, shared by every agent (FgActor, w1 [hidden][D]).  Step 0 acts on the observation of
 * the current state, step k on the one step k-1 returned (after the device auto-reset, when params->auto_reset is set).
 * State pointers, outputs and obs_every as fg_rollout_scenario's (obs may be NULL: not written); act_out [K][B][N][2] is an
 * OUTPUT (the actions taken, required, 8-byte aligned), and fg_rollout_scenario driven by it from the same state returns the
 * same bits.  log_std [2] / logp [K][B][N] (NULL: not written) as in fg_rollout_hd_actor_sample, the same eps draws
 * (fg_actor_noise); log_std == NULL is the deterministic actor, and logp must then be NULL.
 * Shapes: the seven (scenario, N, landmarks, obstacles, num_obs) the one-env-per-lane kernel is built for - basic (3,3,0),
 * partial (5,5,0,3) and (3,5,0,3), range (4,4,0) and (3,4,0), obstacle (4,4,3) and (3,4,3); any other returns
 * FG_ERR_UNSUPPORTED_N.  agent_props, comm_state, scenario->variant == 1 or an unsupported hidden return FG_ERR_BAD_ARG;
 * there is no fall-back inside the library.  B == 0 returns FG_OK without a launch. */
int fg_rollout_scenario_actor(const FgParams* params, const FgScenario* scenario, const FgActor* actor, const float* log_std,
                              int B, int N, int K, float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                              float* landmarks, float* obst_pos, float* obst_vel, int32_t* step,
                              float* obs, float* reward, float* indiv_reward, uint8_t* done, float* act_out, float* logp,
                              int obs_every, void* stream);
/* Dry run of fg_rollout_scenario_actor: same checks and status codes (those on the state and output pointers apart), names
 * the scn_lane_actor<KIND,N,L,M,NBR,H> or scn_lane_actor_gauss<...> instantiation and its launch geometry.  Touches no
 * device; log_std is only checked for NULL and alignment. */
int fg_describe_scenario_actor_launch(const FgParams* params, const FgScenario* scenario, const FgActor* actor,
                                      const float* log_std, int B, int N, int K, int obs_every, char* out, int out_len);

/* Discounted returns of C candidate action sequences, each run for K steps from the CURRENT state of every env, in ONE launch
 * (returns_kernel<N,G,T>): what a planner (random shooting, CEM, MPPI) needs from the simulator.  For every (candidate c, env b)
 * the launch runs the K steps fg_rollout_hd runs on act[c] ([K][B][N][2]) with auto-reset off - the same World.step and reward,
 * bit for bit - from env b's positions, velocities, ideal shape, ideal velocity and step counter, and keeps, per agent i,
 *     d_0 = 1, d_{k+1} = d_k * gamma;   R_k = R_{k-1} + d_k * r_k   for k < steps[b],   R_{-1} = 0
 * in fp32 with every product and every sum rounded on its own (no fused multiply-add): ret [C][B][N] with r = the shared
 * reward (fg_rollout_hd's reward_seq), indiv_ret [C][B][N] (NULL: not written) with r = the individual one (indiv_seq).  A step
 * counts while no earlier step of the launch has set the done flag; the step that sets it counts, nothing after it does:
 *     steps[b] = min(K, max(1, world_length - step[b]))          ([B] int32, NULL: not written; the same for every candidate)
 * EVERY STATE POINTER IS const AND NEVER WRITTEN: state, step counters, ideal shape and velocity stay as they are, no reset is
 * drawn and no RNG counter is read or advanced.  params->auto_reset, rng_offset and rng_offset_dev are ignored.
 * Buffers: fp32 / int32 in DEVICE memory; act, ideal_shape and ideal_vel 8-byte aligned, the others 4-byte aligned.
 * Checks in this order, each with one fixed message: params (NULL, its values); FG_ERR_BAD_ARG for B < 0, K < 1 or C < 1, for a
 * gamma that is not a finite number in [0, 1], and for World options, communication or per-agent properties in params (walls,
 * u_noise, max_speed, accel, agent_props, comm_state: not supported, there is no fall-back inside the library);
 * FG_ERR_UNSUPPORTED_N for an N other than 3, 4, 8, 9, 16, 25, 27, 32; FG_ERR_BAD_ARG for B * C >= 2^31; B == 0 returns FG_OK
 * without a launch; then FG_ERR_BAD_ARG for a NULL required pointer and FG_ERR_ALIGNMENT. */
int fg_rollout_hd_returns(const FgParams* params, int B, int N, int K, int C, float gamma,
                          const float* pos_x, const float* pos_y, const float* vel_x, const float* vel_y,
                          const float* ideal_shape, const float* ideal_vel, const int32_t* step,
                          const float* act, float* ret, float* indiv_ret, int32_t* steps, void* stream);
/* Dry run of fg_rollout_hd_returns: the same checks and status codes (those on the buffers and on gamma apart), then
 * "returns_kernel<N,G,T> grid W block T lds L; " in `text` (cap bytes): G lanes per (candidate, env) pair, T / G pairs per
 * workgroup, W = ceil(B C / (T / G)) workgroups.  B == 0: FG_OK and an empty text.  Touches no device. */
int fg_describe_returns_launch(const FgParams* params, int B, int N, int K, int C, char* text, int cap);

/* ---- A sampling planner's candidates (MPPI, random shooting) without a candidate tensor ----
 * Candidate c's action for agent i of env b at step k of a plan is
 *     u = mean[k][b][i] + sigma * eps          (one rounded product, one rounded sum per component; never an fma)
 *     u = min(max(u, -clip), clip)             where clip > 0; clip <= 0: no clamp
 * with eps the unit normal pair of the planner's own counter stream: the Box-Muller (fp32, words 0 and 1, as the motor noise)
 * of the Philox4x32-10 block with key params->seed and counter
 *     {b + params->env_index_base, 0x40000000 | c << 12 | i, lo32(noise_offset + k), hi32(noise_offset + k)}.
 * Stream code (counter word 1, top three bits): 010 - beside reset and landmarks 000, obstacles 001, Gumbel 011, motor noise
 * 100, actor noise 101, communication 110, ideal velocity 111.  Limits: N <= 2^12 (i in bits 0-11), C <= 2^17 (c in bits
 * 12-28); every planner entry returns FG_ERR_BAD_ARG beyond them.  noise_offset is the CALLER'S counter, passed by value
 * (frozen when a launch is captured into a graph): params->rng_offset and rng_offset_dev are ignored, so planning never moves
 * the env's RNG, and a caller that advances noise_offset by K per plan never draws a number twice.  The three entries below
 * draw the same bits for the same (seed, env_index_base, noise_offset, c, k, b, i).
 * Their common checks, after params: FG_ERR_BAD_ARG for B < 0, K < 1, C < 1, N outside 1 .. 2^12, C > 2^17 or a sigma that
 * is not a finite number >= 0. */

/* fg_rollout_hd_returns with the candidates drawn inside the launch (returns_sampled_kernel<N,G,T>: returns_kernel's
 * geometry, step and recurrence - the results are, bit for bit, those of fg_rollout_hd_returns on the tensor
 * fg_plan_candidates writes).  mean [K][B][N][2] (required, 8-byte aligned) is shared by an env's C candidates; every other
 * buffer, check, status code and their order are fg_rollout_hd_returns' (under this entry's name), followed by the planner
 * checks above, before the pointers. */
int fg_rollout_hd_returns_sampled(const FgParams* params, int B, int N, int K, int C, float gamma, uint64_t noise_offset,
                                  float sigma, float clip,
                                  const float* pos_x, const float* pos_y, const float* vel_x, const float* vel_y,
                                  const float* ideal_shape, const float* ideal_vel, const int32_t* step,
                                  const float* mean, float* ret, float* indiv_ret, int32_t* steps, void* stream);
/* Dry run of fg_rollout_hd_returns_sampled: fg_describe_returns_launch's checks and status codes, FG_ERR_BAD_ARG for
 * C > 2^17, then "returns_sampled_kernel<N,G,T> grid W block T lds L; ".  Touches no device. */
int fg_describe_returns_sampled_launch(const FgParams* params, int B, int N, int K, int C, char* text, int cap);

/* The candidates as a tensor: act_out [C][K][B][N][2] (required, 8-byte aligned), one element-wise launch for any
 * 1 <= N <= 2^12.  mean [K][B][N][2] or NULL = zeros; with mean NULL, sigma = 1 and clip = 0 act_out holds the unit draws
 * themselves.  World options in params are not looked at.  B == 0 returns FG_OK without a launch. */
int fg_plan_candidates(const FgParams* params, int B, int N, int K, int C, uint64_t noise_offset, float sigma, float clip,
                       const float* mean, float* act_out, void* stream);

/* MPPI's update without the candidate tensor.  For every (k, b, i), in fp32 and over c in ascending order:
 *     m = max_c ret[c][b][i];   w_c = exp((ret[c][b][i] - m) / lambda);   new = (sum_c w_c u_c) / (sum_c w_c)
 * with u_c the candidate action above, drawn again from mean_in [K][B][N][2].  new goes to mean_out[k - shift] for
 * k >= shift; with shift = 1 step K - 1's value also goes to mean_out[K - 1] (the plan moves on one step, its last step
 * repeated); step 0's value goes to act_out [B][N][2] (NULL: not written) - the action to take now.  ret [C][B][N] is what
 * the returns entries write (4-byte aligned); mean_in, mean_out, act_out 8-byte aligned.
 * After the common checks: FG_ERR_BAD_ARG for a lambda that is not a finite number > 0 and for a shift other than 0 or 1;
 * B == 0 returns FG_OK; then FG_ERR_BAD_ARG for a NULL ret / mean_in / mean_out, FG_ERR_ALIGNMENT, and FG_ERR_BAD_ARG
 * where the K B N float2 of mean_out overlap those of mean_in (a thread writes another thread's input row), and where
 * mean_out or act_out overlaps ret, act_out overlaps mean_in, or the two outputs overlap each other (outputs are written
 * while other threads still read the inputs). */
int fg_plan_mppi_update(const FgParams* params, int B, int N, int K, int C, uint64_t noise_offset, float sigma, float clip,
                        float lambda, const float* ret, const float* mean_in, float* mean_out, float* act_out, int shift,
                        void* stream);

/* ---- ... with a sigma per step, env, agent and component: the cross-entropy method (CEM) ----
 * The three entries below take std [K][B][N][2] (laid out like mean; required, 8-byte aligned) where the entries above take
 * the scalar sigma:
 *     u = mean[k][b][i] + std[k][b][i] * eps   per component (one rounded product, one rounded sum; never an fma), clamped
 * with the same eps, stream code, noise_offset + k rule and limits.  A std filled with float32(sigma) gives the scalar
 * entries' bits.  THE CALLER'S CONTRACT: every element of std is finite and >= 0 - the library cannot look into device
 * memory.  Their common checks are those above without the one on sigma. */

/* fg_plan_candidates with the sigma tensor.  mean NULL = zeros. */
int fg_plan_candidates_std(const FgParams* params, int B, int N, int K, int C, uint64_t noise_offset, float clip,
                           const float* mean, const float* std, float* act_out, void* stream);

/* fg_rollout_hd_returns_sampled with the sigma tensor (returns_sampled_std_kernel<N,G,T>: the same geometry, step and
 * recurrence, one more 8-byte load per drawn action): bit for bit fg_rollout_hd_returns on the tensor fg_plan_candidates_std
 * writes.  Checks, status codes and their order: fg_rollout_hd_returns_sampled's, under this entry's name, then std. */
int fg_rollout_hd_returns_sampled_std(const FgParams* params, int B, int N, int K, int C, float gamma, uint64_t noise_offset,
                                      float clip,
                                      const float* pos_x, const float* pos_y, const float* vel_x, const float* vel_y,
                                      const float* ideal_shape, const float* ideal_vel, const int32_t* step,
                                      const float* mean, const float* std, float* ret, float* indiv_ret, int32_t* steps,
                                      void* stream);
/* Dry run of fg_rollout_hd_returns_sampled_std: fg_describe_returns_sampled_launch's checks and status codes, then
 * "returns_sampled_std_kernel<N,G,T> grid W block T lds L; ".  Touches no device. */
int fg_describe_returns_sampled_std_launch(const FgParams* params, int B, int N, int K, int C, char* text, int cap);

/* CEM's update without the candidate tensor (plan_cem_update_kernel: one 64-lane wave per (b, i) row).  For every row:
 *   select  the E elites are the E largest of ret[c][b][i], c = 0 .. C-1, under the total order of
 *               key = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000)      (bits of the float, keys compared unsigned)
 *           so -0 < +0, -inf below every finite value, and every bit pattern (NaN included) has a place; equal keys rank
 *           the lower c first.  The selection is exact.
 *   refit   for every step k and component, over the elites' actions u drawn again from (mean_in, std_in), in fp32:
 *               m = mean of u;   v = sum (u - m)^2 / E  (two passes);
 *               mean_new = (1 - alpha) mean_in + alpha m,   std_new = max(sigma_min, (1 - alpha) std_in + alpha sqrt(v))
 *           (the mean is accumulated as mean_in + sum(u - mean_in) / E, so elites that all equal mean_in give it back
 *           exactly).  Two launches on the same inputs give the same bits.
 *   store   mean_new, std_new go to mean_out / std_out [k - shift] for k >= shift; with shift = 1 step K - 1's values also
 *           go to row K - 1 (fg_plan_mppi_update's rule).  mean_new of step 0 goes to act_out [B][N][2] (NULL: not
 *           written); the elites' candidate indices, ascending, to elite_idx [E][B][N] int32 (NULL: not written).
 * After the common checks: FG_ERR_BAD_ARG unless 1 <= E <= C, for an alpha that is not a finite number in (0, 1], a sigma_min
 * that is not a finite number >= 0 and a shift other than 0 or 1; B == 0 returns FG_OK; then FG_ERR_BAD_ARG for a NULL ret /
 * mean_in / std_in / mean_out / std_out, FG_ERR_ALIGNMENT (ret and elite_idx 4-byte, the others 8-byte), and FG_ERR_BAD_ARG
 * where any of mean_out, std_out, act_out, elite_idx overlaps ret, mean_in, std_in or another output. */
int fg_plan_cem_update(const FgParams* params, int B, int N, int K, int C, int E, uint64_t noise_offset, float clip, float alpha,
                       float sigma_min, const float* ret, const float* mean_in, const float* std_in, float* mean_out,
                       float* std_out, float* act_out, int32_t* elite_idx, int shift, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FORMATION_HIP_H_ */
