// formation_hip.hip - hand-written HIP kernels (gfx950 / CDNA4, wave64) for the
// formation_gym hot path, and the C ABI declared in include/formation_hip.h.
//
// What one launch of `step_kernel` does for a group of E environments held by
// one workgroup (reference lines in /root/reference/formation_gym/):
//   phase 1  load SoA state + actions + ideal shape of the group into LDS
//   phase 2  World.step: action force (core.py:228-237, environment.py:216-221),
//            all-pairs soft-contact force on PRE-step positions (core.py:240-262,
//            :289-322), damped Euler integration (core.py:264-277)
//   phase 3  Scenario.reward (formation_hd_env.py:61-75): centroid and mean
//            velocity by wave shuffles, one pass over post-step pairs giving the
//            Hausdorff row/column minima and the collision counts, env-wide
//            max/sum by shuffles (one env never spans a wave unless N > 64)
//   phase 4  optional vec-env auto-reset (env_wrappers.py:14-18)
//   phase 5  Scenario.observation (formation_hd_env.py:52-59) for all N agents:
//            the group's [E][N][6N] block is one contiguous span of global
//            memory, streamed by register-cached row writers or LDS tiles
//            (fg_obs_writers.hpp).
// Rollout launches and single steps at N = 81 / 243 run the same phases split over
// producer and writer waves (fg_rollout_kernels.hpp).
// Observation bytes (24 N^2 per env) dominate traffic; everything else is 53 N + 16.
// There is no dense contraction here, hence no MFMA: the kernel is HBM-store bound.
// (The one exception: the caller's MLP actor inside the closed-loop rollout, fg_actor_rollout_kernel.hpp, on fp32 MFMA.)
//
// Source layout: fg_common.hpp (arguments, LDS layout, reductions, RNG, World options),
// fg_pair_loops.hpp, fg_obs_writers.hpp, fg_step_kernel.hpp, fg_rollout_kernels.hpp,
// fg_policy_kernels.hpp (the reference's demo controller), fg_aux_kernels.hpp (resets) with fg_scn_kernel.hpp (landmark
// scenarios), fg_returns_kernel.hpp (returns of candidate action sequences from the current state),
// fg_planner_kernels.hpp (a sampling planner's candidates: drawn in that launch, as a tensor, MPPI's update); this file holds the host side: variant tables, dispatch and the extern "C" entry
// points.  formation_hip_f64.hip builds the step, rollout and scenario kernels' source in double (tests only).

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <type_traits>
#include <vector>
#include "fg_common.hpp"
#include "fg_pair_loops.hpp"
#include "fg_obs_writers.hpp"
#include "fg_step_kernel.hpp"
#include "fg_rollout_kernels.hpp"
#include "fg_aux_kernels.hpp"
#include "fg_scn_lane_kernel.hpp"
#include "fg_hd_lane_kernel.hpp"
#include "fg_policy_kernels.hpp"
#include "fg_actor_rollout_kernel.hpp"
#include "fg_scn_lane_actor_kernel.hpp"
#include "fg_returns_kernel.hpp"
#include "fg_planner_kernels.hpp"

namespace fg {

// ---------------------------------------------------------------------------
// host side: geometry selection, validation, launches
// ---------------------------------------------------------------------------
static thread_local char g_err[256] = "";

static int fail(int code, const char* fmt, const char* detail = "") {
    snprintf(g_err, sizeof(g_err), fmt, detail);
    return code;
}

struct Geometry { int G, T, E, lds; };

// Dry run of the dispatch (fg_describe_launch): while `g_describe` points at a caller's buffer the launchers below append the
// kernel instantiation and launch geometry they WOULD use and return without touching the device.  A CPU-side test holds a
// committed snapshot of these choices over a grid of shapes (tests/golden/dispatch.json): a threshold that moves changes the
// snapshot, not just a timing somebody may or may not look at.
static thread_local char* g_describe = nullptr;
static thread_local int g_describe_cap = 0;
// describe mode for the calling thread while in scope; off again on every way out
struct DescribeScope {
    DescribeScope(char* out, int cap) { g_describe = out; g_describe_cap = cap; }
    ~DescribeScope() { g_describe = nullptr; g_describe_cap = 0; }
    DescribeScope(const DescribeScope&) = delete;
    DescribeScope& operator=(const DescribeScope&) = delete;
};
static bool describe(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
static bool describe(const char* fmt, ...) {
    if (!g_describe) return false;
    const int used = (int)strlen(g_describe);
    if (used < g_describe_cap - 1) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(g_describe + used, (size_t)(g_describe_cap - used), fmt, ap);
        va_end(ap);
    }
    return true;
}

// A launch goes to the device its DATA lives on: if that is not the calling thread's current device (an env living
// on cuda:1 driven from a thread whose current device is cuda:0), switch for the duration of the call.  A non-NULL
// stream names its device; the NULL stream is "the default stream of whatever device is current", which says nothing
// (torch hands out 0 for the default stream of EVERY device), so there the device is read off the first state pointer
// (hipPointerGetAttributes).  A process that sees one GPU never pays for either query.
static int visible_devices() {
    static const int n = [] { int c = 0; return hipGetDeviceCount(&c) == hipSuccess ? c : 1; }();
    return n;
}
// the device a launch with this stream and this first data pointer belongs to; -1 = cannot tell (stay on the current device)
static int resolve_device(void* stream, const void* data) {
    if (stream) {
        hipDevice_t sdev = -1;
        if (hipStreamGetDevice((hipStream_t)stream, &sdev) == hipSuccess) return (int)sdev;
        (void)hipGetLastError();
        return -1;
    }
    if (data) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, data) == hipSuccess && attr.type == hipMemoryTypeDevice) return attr.device;
        (void)hipGetLastError();                                 // a host / unknown pointer: leave the error state clean
    }
    return -1;
}
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    // `target`: a device resolved earlier (resolve_device; fg_step_hd_plan resolves once, so that a planned step pays no query)
    explicit DeviceGuard(int target) {
        if (target >= 0 && hipGetDevice(&prev) == hipSuccess && prev != target) switched = hipSetDevice(target) == hipSuccess;
    }
    DeviceGuard(void* stream, const void* data) : DeviceGuard(visible_devices() < 2 ? -1 : resolve_device(stream, data)) {}
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// Kernels that need more than the default 64 KiB of dynamic LDS opt in once per (kernel, device): the
// attribute belongs to the device the function is loaded on, and a process may drive several GPUs (one
// thread each: the bookkeeping is atomic).
static hipError_t raise_lds_limit(const void* fn, int lds, std::atomic<unsigned long long>* done_mask) {
    if (lds <= 64 * 1024) return hipSuccess;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if ((done_mask->load(std::memory_order_acquire) >> dev) & 1ull) return hipSuccess;
    const hipError_t err = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (err == hipSuccess) done_mask->fetch_or(1ull << dev, std::memory_order_release);
    return err;
}

// THE launch of this file: the kernel's LDS opt-in (the mask is the kernel's own by construction), the launch, the runtime's
// answer as a status - FG_OK, or FG_ERR_HIP with `fail_fmt`, the caller's name for the launch, around the runtime's text.
// A caller with a dry run (describe) asks it first, so that its describe string stays its own.
template <auto Kernel> static std::atomic<unsigned long long> g_lds_raised{0};
template <auto Kernel, class... A>
static int launch(unsigned grid, int threads, int lds, hipStream_t st, const char* fail_fmt, const A&... args) {
    hipError_t err = raise_lds_limit((const void*)Kernel, lds, &g_lds_raised<Kernel>);
    if (err == hipSuccess) {
        hipLaunchKernelGGL(Kernel, dim3(grid), dim3(threads), lds, st, args...);
        err = hipGetLastError();
    }
    return err == hipSuccess ? FG_OK : fail(FG_ERR_HIP, fail_fmt, hipGetErrorString(err));
}

static int pow2ceil(int x) { int p = 1; while (p < x) p <<= 1; return p; }

// A run-time G in {4, 8, ..., 1024} as a compile-time <G, max(G, 64)> (lanes per env, threads per workgroup: reset_kernel,
// scn_kernel): run(g, t) with both as the `value` of the arguments' types
template <int V> using IntC = std::integral_constant<int, V>;
template <class F>
static int pow2_dispatch(int G, F&& run) {
#define FG_G(GG) if (G == GG) return run(IntC<GG>{}, IntC<(GG < 64 ? 64 : GG)>{});
    FG_G(4) FG_G(8) FG_G(16) FG_G(32) FG_G(64) FG_G(128) FG_G(256) FG_G(512)
#undef FG_G
    return run(IntC<1024>{}, IntC<1024>{});
}

// step_kernel's arguments: the state pointers ahead of `a` (kernarg preload, fg_step_kernel.hpp)
template <auto Kernel>
static int launch_step_kernel(const Args& a, int n_split, int grid, int threads, int lds, hipStream_t st) {
    return launch<Kernel>(grid, threads, lds, st, "kernel launch failed: %s", a.B, n_split, (const float*)a.px, (const float*)a.py,
                          (const float*)a.vx, (const float*)a.vy, (const float*)a.shape, (const float*)a.ivel,
                          (const int32_t*)a.step, a);
}
template <int NC, int G, int T, int E, bool IDX, bool OPTS>
static int launch_v(const Args& a, int grid, int lds, hipStream_t st) {
    const int n_split = a.N | ((E == 1 && a.split > 1 ? a.split : 0) << 16);
    // the single-step instantiation (no step loop, no slot arithmetic) of the plain variants from 27 agents up: 27 x 4096
    // 15.15 -> 15.03 us, 81 x 2048 -1 %; at 3 and 9 agents it is slower (profiles/r02_step/kone.txt)
    constexpr bool HAS_KONE = !IDX && !OPTS && NC >= 27;
    const bool kone = HAS_KONE && a.K == 1 && a.obs_every == 1;
    if (describe("step_kernel<%d,%d,%d,%d,%d,%d,%d> grid %d lds %d%s; ", NC, G, T, E, (int)IDX, (int)OPTS, (int)kone, grid, lds,
                 a.obs_only ? " obs-only" : ""))
        return FG_OK;
    // (each instantiation has its own LDS opt-in; above 64 KiB: run-time N close to 1024, + the per-agent tables of OPTS)
    if (kone) return launch_step_kernel<&step_kernel<NC, G, T, E, false, false, HAS_KONE>>(a, n_split, grid, T, lds, st);
    return launch_step_kernel<&step_kernel<NC, G, T, E, IDX, OPTS>>(a, n_split, grid, T, lds, st);
}

using LaunchFn = int (*)(const Args&, int, int, hipStream_t);
// One entry per (agent count, workgroup shape).  plain / idx (+ landmark-index outputs) / opts (idx + World options
// no reference scenario enables).  min_B: the entry is the default from that batch size up (MI355X sweeps,
// profiles/README.md: a batch that fills the chip many times over streams best with 8 envs per workgroup, a
// single-generation batch prefers one env per wave with spare writer waves).  NC = 0 entries take N at run time.
struct Variant { int NC, G, T, E, min_B; LaunchFn plain, idx, opts; };
#define FG_VARIANT(NC, G, T, E, MINB) {NC, G, T, E, MINB, &launch_v<NC, G, T, E, false, false>, \
                                       &launch_v<NC, G, T, E, true, false>, &launch_v<NC, G, T, E, true, true>}
#define FG_VARIANT_BIG(NC, G, T, E, MINB) {NC, G, T, E, MINB, &launch_v<NC, G, T, E, false, false>, nullptr, nullptr}

// batch-size thresholds of the dispatch below (MI355X sweeps; the profile behind each is named where it is used)
constexpr int FG_SPLIT_MAX_B = 128;        // split step (launch_step) up to this many envs
constexpr int FG_WIDE81_MIN_B = 16384;     // single-step launches at 81 agents take the pipelined kernel from this batch size up
constexpr int FG_WIDE243_MIN_B = 4096;     // single-step launches at 243 agents: below this the pipelined kernel's 4-env batches leave CUs
                                           // idle and one env per workgroup (step_kernel) is up to 3x faster (profiles/r02_step/wide243_min_b.txt)
static const Variant kVariants[] = {
    FG_VARIANT(3, 4, 128, 16, 0), FG_VARIANT_BIG(3, 4, 128, 32, 65536),   // every lane owns an agent: 3 x 262144 35.3 -> 27.8 us (profiles/r02_step/n3_big_batches.txt)
    FG_VARIANT(9, 16, 128, 4, 0), FG_VARIANT_BIG(9, 16, 128, 8, 16384),
    FG_VARIANT(27, 32, 256, 4, 0), FG_VARIANT_BIG(27, 32, 256, 8, 32768),
    FG_VARIANT(81, 128, 128, 1, 0),
    FG_VARIANT(243, 256, 256, 1, 0),
    // the agent counts of the other hierarchies get_action_BFS takes (per_layer 2, 4, 5, 8: __init__.py:49-56): compile-time
    // N with the register-cached rows writer for the plain launch; index outputs / World options take the run-time-N kernels
    FG_VARIANT_BIG(4, 4, 128, 16, 0), FG_VARIANT_BIG(8, 8, 128, 8, 0), FG_VARIANT_BIG(16, 16, 128, 4, 0),
    FG_VARIANT_BIG(25, 32, 256, 4, 0), FG_VARIANT_BIG(32, 32, 256, 4, 0), FG_VARIANT_BIG(64, 64, 256, 2, 0),
    FG_VARIANT_BIG(125, 128, 128, 1, 0),
    FG_VARIANT(0, 4, 64, 16, 0), FG_VARIANT(0, 8, 64, 8, 0), FG_VARIANT(0, 16, 64, 4, 0), FG_VARIANT(0, 32, 128, 4, 0),
    FG_VARIANT(0, 64, 128, 2, 0), FG_VARIANT(0, 128, 128, 1, 0), FG_VARIANT(0, 256, 256, 1, 0),
    FG_VARIANT(0, 512, 512, 1, 0), FG_VARIANT(0, 1024, 1024, 1, 0),
};

// need_full: the launch wants the idx / opts instantiation (only the first entry of an agent count has them)
// generic: the run-time-N instantiation whatever N is (its flat observation writer is the one that knows the
//          communication block of non-silent agents, FgParams.comm_state)
static const Variant* variant_for(int N, int B = 0, bool need_full = false, bool generic = false) {
    if (N < 2 || N > FG_MAX_AGENTS) return nullptr;
    const Variant* best = nullptr;
    for (const Variant& v : kVariants) {
        if (generic || v.NC != N || B < v.min_B || (need_full && !v.opts)) continue;
        if (!best || v.min_B > best->min_B) best = &v;
    }
    if (best) return best;
    const int G = N <= 64 ? (pow2ceil(N) < 4 ? 4 : pow2ceil(N)) : (pow2ceil(N) < 128 ? 128 : pow2ceil(N));
    for (const Variant& v : kVariants)
        if (v.NC == 0 && v.G == G) return &v;
    return nullptr;
}

static bool geometry_for(int N, Geometry* g, int B = 0, bool need_full = false, bool generic = false) {
    const Variant* v = variant_for(N, B, need_full, generic);
    if (!v) return false;
    g->G = v->G; g->T = v->T; g->E = v->E;
    g->lds = step_lds_bytes(N, v->E, false);
    return true;
}

// the N checks: any scenario-free launch takes 2 ... 1024 agents, formation_hd_env's observation and reward need 3
static int generic_n_check(int N) {
    return N < 2 || N > FG_MAX_AGENTS ? fail(FG_ERR_UNSUPPORTED_N, "N must be in [2, 1024]%s") : FG_OK;
}
static int hd_n_check(int N) {
    return N < 3 || N > FG_MAX_AGENTS ? fail(FG_ERR_UNSUPPORTED_N, "formation_hd_env needs 3 <= N <= 1024%s") : FG_OK;
}

static bool world_options_set(const FgParams& p) {
    return p.num_walls > 0 || p.u_noise > 0.f || p.max_speed > 0.f || p.accel > 0.f || p.agent_props || p.comm_state;
}

static int launch_step(Args a, hipStream_t st) {
    Geometry g;
    const bool opts = world_options_set(a.p);
    const bool idx = a.near_lm || a.near_ag || a.hd_idx;
    const bool generic = a.p.comm_state != nullptr;
    if (const int rc = generic_n_check(a.N)) return rc;
    const Variant* v = variant_for(a.N, a.B, opts || idx, generic);      // (never NULL: the run-time-N entries cover every N in range)
    geometry_for(a.N, &g, a.B, opts || idx, generic);
    if (opts) g.lds = step_lds_bytes(a.N, g.E, true);    // + per-agent mass / size / flags, per-env comm states
    a.coll_scale = (float)((double)a.p.collide_thresh / (double)a.p.dist_min);
    const int grid = (a.B + g.E - 1) / g.E;
    // Split step: more than 64 agents (one env per workgroup) and fewer envs than half the chip's CUs.  One workgroup per
    // env would leave most CUs idle during the observation stream, which is 99 % of the bytes; so the fused kernel runs
    // WITHOUT the observation (state, reward, done, reset) and a second launch of S workgroups per env streams the
    // observation from the final state - the very values the fused kernel holds in LDS, hence the same bits
    // (243 x 64: 43.4 -> 37.4 us, 256 x 64: 69 -> 41, 1024 x 64: 581 -> 394-448; neutral at 81 agents; 243 x 128 loses 8 %,
    // hence 96 there: profiles/r02_step/split_step.txt)
    if (g.E == 1 && a.K == 1 && a.do_phys && a.do_post && a.obs && a.B <= (a.N == 243 ? (FG_SPLIT_MAX_B * 3) / 4 : FG_SPLIT_MAX_B)) {
        int S = 256 / a.B;
        if (S > 8) S = 8;
        Args a1 = a; a1.obs = nullptr;
        const int rc = (opts ? v->opts : idx ? v->idx : v->plain)(a1, grid, g.lds, st);
        if (rc) return rc;
        Args a2 = a;
        a2.do_phys = 0; a2.obs_only = 1; a2.split = S; a2.p.auto_reset = 0;
        a2.rew = nullptr; a2.indiv = nullptr; a2.done = nullptr; a2.near_lm = nullptr; a2.near_ag = nullptr; a2.hd_idx = nullptr;
        return (generic ? v->opts : v->plain)(a2, grid * S, g.lds, st);   // the communication block lives in the OPTS instantiation
    }
    return (opts ? v->opts : idx ? v->idx : v->plain)(a, grid, g.lds, st);
}

// 64 < N <= 256: producer / writer pipelined kernel (rollout: over steps; single step: over env batches)
// PER > 0: closed loop with the PER-ary demo controller inside the kernel (fg_rollout_hd_policy)
template <int NC, int A, int E, int TW, int PER, bool BATCHES = false>
static int launch_wide_v(Args a, hipStream_t st) {
    a.groups = 1;
    if constexpr (BATCHES) {
        // env batches per workgroup: enough to overlap batch g+1's pair loops with batch g's store
        // stream, few enough to keep every CU busy (one workgroup per CU; MI355X sweep, profiles/README.md)
        const int batches = (a.B + E - 1) / E;
        a.groups = batches / 256;
        if (a.groups < 1) a.groups = 1;
        if (a.groups > 64) a.groups = 64;
    }
    const int grid = (a.B + E * a.groups - 1) / (E * a.groups);
    const int lds = E * roll_block_floats(NC) * (int)sizeof(float) +
                    (PER > 0 ? E * policy_block_units(NC) * (int)sizeof(float2) : 0);
    if (describe("rollout_kernel_wide<%d,%d,%d,%d,%d,%d> grid %d lds %d groups %d; ", NC, A, E, TW, PER, (int)BATCHES, grid, lds, a.groups))
        return FG_OK;
    return launch<&rollout_kernel_wide<NC, A, E, TW, PER, BATCHES>>(grid, E * 64 + TW, lds, st, "pipelined launch failed: %s", a);
}
// 4 envs (= producer waves) and 4 writer waves per workgroup (MI355X sweeps: profiles/README.md, profiles/r03_wide/)
template <int NC, int PER>
static int launch_wide(const Args& a, hipStream_t st) {
    static_assert(NC > 64 && NC <= 256, "one producer wave per env, up to 4 agents per lane");
    constexpr int A = (NC + 63) / 64;
    // 243 agents, at most 256 envs: one env per workgroup spreads the batch over more CUs (243 x 256 x 8: 103 -> 82 us/step,
    // 243 x 64: 90 -> 78; at 81 agents the producer wave's own chain, ~15 us per step, is the bound whatever the geometry:
    // profiles/r03_wide/ab_wide_small_batches.txt)
    // a single step (K == 1) of the open loop pipelines over env batches inside the workgroup (fg_step_hd at 81 / 243 agents)
    if constexpr (PER == 0 && (NC == 81 || NC == 243))
        if (a.K == 1) return launch_wide_v<NC, A, 4, 256, 0, true>(a, st);
    if constexpr (NC == 243)
        if (a.K > 1 && a.B <= 256) return launch_wide_v<243, 4, 1, 256, PER>(a, st);
    return launch_wide_v<NC, A, 4, 256, PER>(a, st);
}

// N <= 64, K >= 2: producer / writer pipelined rollout kernel
template <int NC, int G, int TP, int TW, int E, int WR, int PER, bool STREAM = false>
static int launch_roll_v(const Args& a, hipStream_t st) {
    const int grid = (a.B + E - 1) / E;
    constexpr int lds = roll_lds_bytes<NC, TW, E, WR, PER>();     // env blocks, writer tiles, controller tables, reward hand-over
    if (describe("rollout_kernel<%d,%d,%d,%d,%d,%d,%d,%d> grid %d lds %d; ", NC, G, TP, TW, E, WR, PER, (int)STREAM, grid, lds)) return FG_OK;
    return launch<&rollout_kernel<NC, G, TP, TW, E, WR, PER, STREAM>>(grid, TP + TW, lds, st, "rollout launch failed: %s", a);
}
// writer of the pipelined kernels per agent count: 1 + rows per LDS tile (the rows must divide N: 9 of 27 and 9, 5 of 25,
// 8 of 16 and 32), 0 = register-cached rows (few agents: a tile is too small to pay; 64 agents: a row is a wave)
constexpr int roll_writer(int n) { return n == 9 ? FG_WR_GATHER : n == 27 ? 10 : n == 25 ? 6 : (n == 16 || n == 32) ? 9 : 0; }

// ---- which instantiation a (agents, batch, buffer) gets: ONE rule table per agent-count class --------------------------------
// A rule = a batch range, conditions on the observation buffer, the instantiation, and the measurement that put the threshold
// where it is.  The FIRST rule that applies is taken; a row whose instantiation does not exist for this (agents, per) - `on`
// false - is skipped, every table ends with a catch-all.  tests/golden/dispatch.json holds what these tables answer over a grid
// of shapes (tests/test_dispatch_snapshot.py): a moved threshold is a diff of that file.
//   rollout_kernel<NC, G, TP, TW, E, WR, PER, STREAM>: G lanes per env, TP producer + TW writer threads, E envs per workgroup,
//   WR the observation writer (0 rows, FG_WR_GATHER, else 1 + rows per LDS tile), STREAM the HBM-streaming form of the writer
using RollFn = int (*)(const Args&, hipStream_t);
enum : unsigned {
    R_HBM = 1u,          // the launch's observation buffer does not fit the 256 MiB Infinity Cache (> 400 MB)
    R_CACHED = 2u,       // ... it does
    R_PLACED = 4u,       // FgParams.obs_placed: the buffer was composed of chunks spread over the device's memory (fg_arena_*)
    R_BEYOND_IC = 16u,   // ... it exceeds the Infinity Cache at all (> 260 MB): the late-round-5 geometry rules, which win from there on
                         // (profiles/r05_hbm_threshold_ab.txt: 9 x 8192 x 20 = 318 MB 3.30 -> 3.21 us/step, 8 x 16384 x 10 5.01 -> 4.59;
                         // at 100-150 MB they lose 3-4 %)
    R_FILL32 = 8u,       // workgroups of 32 envs, one per CU at a time (1024 threads), fill their generations of 256 well enough
                         // (run_roll_rules)
    R_FILL32B = 32u,     // the same for the 512- / 768-thread 32-env workgroups of 8 agents: whole generations of 256, a last one at least
                         // half full, or six and more (profiles/r05_fill_rule_ab.txt: 1.12 / 1.25 / 2.25 generations lose 0-11 %)
};
struct RollRule {
    int b_lo, b_hi;      // batch sizes the rule covers (inclusive)
    unsigned need;       // R_* conditions, all of them
    RollFn fn;           // nullptr: no such instantiation for this (agents, per)
    const char* why;     // the measurement behind the threshold
};
constexpr int B_ANY = 0x7fffffff;
template <bool ON, int NC, int G, int TP, int TW, int E, int WR, int PER, bool STREAM = false>
constexpr RollFn roll_fn() {
    if constexpr (ON) return &launch_roll_v<NC, G, TP, TW, E, WR, PER, STREAM>;
    else return nullptr;
}
template <size_t R>
static int run_roll_rules(const RollRule (&rules)[R], const Args& a, hipStream_t st) {
    const double obs_bytes = (double)(a.K / a.obs_every) * a.B * (double)a.obs_pitch * 8.0;
    const bool hbm = obs_bytes > 400e6, beyond_ic = obs_bytes > 260e6;
    for (const RollRule& r : rules) {
        if (!r.fn || a.B < r.b_lo || a.B > r.b_hi) continue;
        if (((r.need & R_HBM) && !hbm) || ((r.need & R_CACHED) && hbm) || ((r.need & R_PLACED) && !a.p.obs_placed)) continue;
        if ((r.need & R_BEYOND_IC) && !beyond_ic) continue;
        if (r.need & R_FILL32B) {
            const int wgs = (a.B + 31) / 32, full = wgs / 256, rest = wgs % 256;
            if (!(rest == 0 || rest >= 128 || full >= 6)) continue;
        }
        if (r.need & R_FILL32) {
            // generations of 256 workgroups (one 1024-thread workgroup per CU): whole ones, a last one at least three quarters full,
            // or six and more - profiles/r05_fill_rule_ab.txt: 1.00 +8 %, 1.12 -10 %, 1.25 -7 %, 1.50 -2 %, 1.75 +12 % (placed: +7 %),
            // 2.25 -3 %, 3.75 +9 % (placed: +2 %), 6.00 +7 %; half-full last generations (2.50 +1 %, 3.50 +2.5 %, 4.50 +3 % on ordinary
            // allocations) lose on placed buffers (3.50: -6.5 % on two boxes) and are left out
            const int wgs = (a.B + 31) / 32, full = wgs / 256, rest = wgs % 256;
            if (!(rest == 0 || rest >= 192 || full >= 6)) continue;
        }
        return r.fn(a, st);
    }
    return fail(FG_ERR_UNSUPPORTED_N, "no rollout rule for this shape%s");       // (unreachable: every table ends with a catch-all)
}

// up to 8 agents (3, 4, 8): one wave of producers, two writer waves with the rows writer (rows of 9 units keep 9 of a wave's
// 64 lanes busy; one writer wave was the bottleneck: 3 x 1024 x 20 2.28 -> 1.36 us/step, 3 x 16384 2.48 -> 1.63, 3 x 65536
// 7.46 -> 7.05; four waves lose from 16384 envs up)
template <int NC, int PER>
static int launch_roll_8(const Args& a, hipStream_t st) {
    constexpr int G = NC <= 4 ? 4 : 8, E = 64 / G;
    constexpr bool N8 = NC == 8, OPEN = PER == 0;
    static constexpr RollRule rules[] = {
        {4096, 5119, R_HBM, roll_fn<N8 && OPEN, NC, G, 128, 512, 128 / G, FG_WR_GATHER, PER>(),
         "profiles/r04_writers_ab.txt: one workgroup per CU into a buffer beyond the Infinity Cache, 16 envs and eight writer waves "
         "per workgroup - 8 x 4096 x 120 1.69 -> 1.36 us/step (the writer waves bound it); profiles/r05_8x32_ab.txt: with the span form of "
         "the gather writer instead of LDS tiles 8 x 4096 x 160 1.152 -> 1.057 (0.74 -> 0.81 real), 8 x 4500 2.18 -> 1.98"},
        {8192, 49152, R_BEYOND_IC | R_FILL32B, roll_fn<N8 && OPEN, NC, G, 256, 512, 32, FG_WR_GATHER, PER>(),
         "profiles/r05_8x32_ab.txt: 32 envs, 4 producer and 8 writer waves per workgroup - 8 x 8192 x 80 2.36 -> 2.22 us/step, 8 x 16384 "
         "4.74-4.97 -> 4.28-4.39, 8 x 24576 6.96 -> 6.48, 8 x 32768 8.99 -> 8.61, 8 x 49152 13.36 -> 13.10 (0.80 of 8 TB/s in real bytes); "
         "8 x 65536 stays with the small workgroups (17.6-17.8 vs 17.9-18.1)"},
        {12288, B_ANY, R_FILL32B, roll_fn<N8 && PER == 2, NC, G, 256, 256, 32, FG_WR_GATHER, PER>(),
         "profiles/r05_8x32_ab.txt: closed loop, 32 envs, 4 + 4 waves per workgroup - 8 x 12288 6.18 -> 3.90 us/step, 8 x 16384 6.88 -> 4.65, "
         "8 x 24576 9.54 -> 7.39, 8 x 32768 10.64 -> 9.42, 8 x 65536 20.1-20.4 -> 18.95-19.4 (0.50-0.69 -> 0.72-0.74 real); 8 x 8192 keeps the "
         "small workgroups (2.92 vs 3.03)"},
        {12288, 49152, R_FILL32B, roll_fn<N8 && PER == 8, NC, G, 256, 256, 32, FG_WR_GATHER, PER>(),
         "profiles/r05_8x32_ab.txt: the one-level 8-ary controller - 8 x 16384 9.93 -> 6.52 us/step, 8 x 24576 13.49 -> 9.87, 8 x 32768 14.65 -> "
         "13.28, 8 x 49152 21.25 -> 20.35; equal at 65536 (27.9 vs 28.2)"},
        {32768, B_ANY, 0, roll_fn<N8 && PER == 8, NC, G, 64, 64, E, FG_WR_GATHER, PER>(),
         "profiles/r05_r8_ab.txt: closed loop over many workgroup generations is bound by the producers' chain (controller + physics, "
         "~3.6 us per step); ONE writer wave leaves room for more resident producer waves - 8 x 65536 22.7 -> 20.9 us/step; at 8192 "
         "envs two writer waves stay ahead (3.17 vs 3.50)"},
        {4096, B_ANY, 0, roll_fn<N8, NC, G, 64, 128, E, FG_WR_GATHER, PER>(),
         "profiles/r04_gather_ab.txt: an env's 1536 bytes as one contiguous span of 16-byte stores instead of rows in 64- / 128-byte "
         "pieces (LDS tiles: 8 x 65536 23.3 -> 20.2 us/step, 8 x 8192 3.14 -> 2.69; the gather writer since: 18.9 -> 18.6, equal at "
         "8192; closed loop 23.2 -> 22.7); 8 x 1024 is bound by the producers' chain and keeps the rows writer (1.09 vs 1.48)"},
        {0, B_ANY, 0, roll_fn<true, NC, G, 64, 128, E, 0, PER>(), "the default of this class (comment above)"},
    };
    return run_roll_rules(rules, a, st);
}
// 9 ... 16 agents: a batch of <= 4096 envs is bound by the producers' dependent chain and wants many small workgroups with
// the row writer; larger batches are store-bound and want whole 128-byte lines per workgroup with the LDS-tile writer.
template <int NC, int PER>
static int launch_roll_16(const Args& a, hipStream_t st) {
    constexpr int WR = roll_writer(NC);
    constexpr bool N9 = NC == 9, OPEN = PER == 0;
    // 9 agents into a rollout buffer beyond the Infinity Cache (128 steps of 4096 envs: 1 GB).  Cycle stamps inside the kernel
    // (profiles/r04_trace_ab.txt) showed the writer waves, not the producers' chain and not the memory, bounding it: 5400-5700
    // cycles per step for four waves with the tile writer against 2800 for the producers.  Hence the gather writer
    // (fg_obs_writers.hpp; 9 x 8192 3.40 -> 3.10 us/step, 9 x 16384 6.8 -> 6.3, profiles/r04_gather_ab.txt) and, while a
    // workgroup has a CU to itself, more writer waves per env
    static constexpr RollRule rules[] = {
        {1025, 2048, R_HBM, roll_fn<N9 && OPEN, NC, 16, 128, 256, 8, WR, PER>(),
         "profiles/r04_writers_ab.txt, r04_gather_geom.txt: 9 x 2048 x 250 1.47 -> 1.31 us/step"},
        {2049, 4096, R_HBM, roll_fn<N9 && OPEN, NC, 16, 256, 512, 16, WR, PER>(),
         "profiles/r04_writers_ab.txt, r04_gather_geom.txt: 9 x 4096 x 128 2.42 -> 1.83 us/step (1.43 since: profiles/r05_9x4096_rollout.md)"},
        {2049, 4096, R_HBM, roll_fn<N9 && !OPEN, NC, 16, 256, 256, 16, WR, PER>(),
         "profiles/r04_writers_ab.txt: the closed loop's controller tables leave LDS for four writer waves"},
        {8192, B_ANY, R_BEYOND_IC | R_FILL32, roll_fn<N9 && OPEN, NC, 16, 512, 512, 32, WR, PER>(),
         "profiles/r05_9x32_ab.txt: 32 envs, 8 producer and 8 writer waves per workgroup - 9 x 8192 x 64 2.97 -> 2.84 us/step, 9 x 16384 5.69 -> "
         "5.44, 9 x 32768 11.49 -> 11.10, 9 x 65536 23.9 -> 23.3 (0.76 -> 0.78-0.795 of 8 TB/s in real bytes); a batch that leaves the last "
         "generation half empty loses (9 x 12288: 4.42 -> 4.97)"},
        {8192, 32768, R_BEYOND_IC, roll_fn<NC == 16 && OPEN, NC, 16, 256, 512, 16, WR, PER>(),
         "profiles/r05_16x_ab.txt: eight writer waves per 16 envs - 16 x 8192 x 24 8.61 -> 8.10 us/step, 16 x 16384 16.91 -> 16.03, 16 x 32768 "
         "33.8 -> 33.55 (0.77-0.79 -> 0.80-0.83 of 8 TB/s in real bytes); 16 x 65536 and the closed loop keep four (69.8 vs 73.7; 16.5 vs 17.25)"},
        {8192, B_ANY, 0, roll_fn<true, NC, 16, 256, 256, 16, WR, PER>(), "profiles/README.md (round 2 sweeps): store-bound, whole lines per workgroup"},
        {4097, B_ANY, 0, roll_fn<true, NC, 16, 128, 128, 8, WR, PER>(), "profiles/README.md (round 2 sweeps)"},
        {0, B_ANY, 0, roll_fn<true, NC, 16, 64, 128, 4, 0, PER>(), "the producers' chain bounds it: many small workgroups, rows writer"},
    };
    return run_roll_rules(rules, a, st);
}
// 17 ... 32 agents (25, 27, 32).  Defaults from the MI355X sweeps at 27 agents (profiles/README.md): 16 envs per workgroup =
// 8 producer + 4 writer waves, one workgroup per CU at 4096 envs, LDS-tile writer.
template <int NC, int PER>
static int launch_roll_32(const Args& a, hipStream_t st) {
    constexpr int WR = roll_writer(NC);
    constexpr bool POLICY = PER > 0, N27 = NC == 27;
    static constexpr RollRule rules[] = {
        // Batches that do not fill the chip with 16-env workgroups (4096 envs = 256 workgroups = one per CU): fewer envs per
        // workgroup, so that the batch still spreads over the CUs
        {0, 512, 0, roll_fn<N27, NC, 32, 64, 256, 2, WR, PER>(),
         "profiles/r03_wide/ab_27_small_batches_*.txt: 27 x 512 x 20 9.1 -> 2.6 us/step, 27 x 256 9.1 -> 2.6"},
        {0, 1024, 0, roll_fn<true, NC, 32, 128, 256, 4, WR, PER>(), "profiles/r03_wide/ab_27_small_batches_*.txt: 27 x 1024 x 20 9.2 -> 3.4 us/step"},
        {0, 2048, 0, roll_fn<N27 && POLICY, NC, 32, 256, 256, 8, WR, PER>(), "profiles/r03_wide/ab_27_small_batches_*.txt: 27 x 2048 8.0 -> 6.0-6.5 us/step"},
        {0, 2048, R_HBM, roll_fn<N27 && !POLICY, NC, 32, 256, 512, 8, WR, 0, true>(),
         "profiles/r03_wide/ab_27_small_batches_*.txt: 27 x 2048 8.0 -> 6.0-6.5 us/step, placed or not; the HBM-streaming form of the tile writer"},
        {0, 2048, R_CACHED, roll_fn<N27 && !POLICY, NC, 32, 256, 512, 8, WR, 0, false>(), "... and its plain form while the buffer stays in the Infinity Cache"},
        // (27 x 2560 and up are faster with 16 envs per workgroup)
        // 25 and 32 agents into buffers beyond the Infinity Cache: the rows writer with four writer waves (their 5- and 8-row tiles
        // are smaller than 27's 9-row ones, and the streaming form's pacing was tuned on those)
        {4096, B_ANY, R_HBM | R_PLACED, roll_fn<!POLICY && !N27, NC, 32, 512, 256, 16, 0, 0>(),
         "profiles/r05_25_32_ab.txt: placed buffers - 25 x 4096 x 20 10.71 -> 10.44 us/step, 25 x 8192 21.29 -> 20.23, 32 x 4096 15.50 -> 15.20"},
        {4096, B_ANY, R_BEYOND_IC, roll_fn<!POLICY && NC == 32, NC, 32, 512, 256, 16, 0, 0>(),
         "profiles/r05_25_32_ab.txt: ordinary allocations - 32 x 4096 x 20 18.56 -> 18.00 us/step"},
        {0, B_ANY, R_HBM, roll_fn<POLICY, NC, 32, 512, 512, 16, 0, PER>(),
         "profiles/r03_wide/ab_closed_loop_*: the closed-loop instantiation cannot hold 16 tiles beside its controller tables; it takes its "
         "8 writer waves with the rows writer - 11.7 vs 13.35 us/step on a placed buffer; profiles/r05_hint_audit.txt: on an ordinary "
         "allocation as well (27 x 2560 x 32 13.05 -> 8.44, 27 x 8192 27.6 -> 26.0, 25 x 4096 12.8 -> 11.9; 27 x 4096 equal)"},
        {0, B_ANY, R_HBM | R_PLACED, roll_fn<!POLICY, NC, 32, 512, 512, 16, WR, 0, true>(),
         "profiles/r03_wide/ab_27_writers_*.txt: a buffer composed of chunks spread over the device's memory takes the stream of 8 paced writer "
         "waves - 27 x 4096 x 20 11.6-11.8 us/step against 12.9 with 4, 27 x 8192 23.3-23.5 against 25.9-26.4, 27 x 16384 47.6-48.4 against "
         "48.7-49.4; on an ordinary allocation 8 waves lose (13.2-14.4 against 12.75, round 2)"},
        {0, 3072, R_HBM, roll_fn<!POLICY, NC, 32, 512, 512, 16, WR, 0, true>(),
         "profiles/r03_wide/ab_27_mid_batches.txt: ... and so does any buffer while fewer than ~200 of the 256 CUs have a workgroup (a "
         "workgroup's own store rate is the bound then): 27 x 2560 x 37 on an ordinary allocation 12.4 -> 8.1 us/step, 27 x 3072 12.5 -> 10.7 "
         "(27 x 3584 equal, 27 x 4000 12.8 vs 14.0 stays with 4)"},
        {8192, B_ANY, R_HBM, roll_fn<!POLICY && N27, NC, 32, 512, 512, 16, WR, 0, true>(),
         "profiles/r05_hint_audit.txt, r05_25_32_ab.txt: from 8192 envs the eight paced writer waves win on an ordinary allocation too - "
         "27 x 8192 x 10 26.0-26.2 -> 25.2-25.5 us/step, 27 x 16384 49.6 -> 48.8-49.1 (27 x 4096 keeps four: 12.8 vs 13.1-13.2)"},
        {0, 16383, R_HBM, roll_fn<!POLICY && N27, NC, 32, 512, 256, 16, WR, 0, true>(),
         "profiles/README.md (round 2): line ownership + paced stores for batches of a few workgroup generations whose buffer does not fit the "
         "Infinity Cache; 27 agents only - profiles/r05_25_32_ab.txt: at 25 agents on an ordinary allocation this form ran 15.1 us/step (4096 "
         "envs) and 30.8 (8192) where the plain tile writer below runs 11.5 and 23.5"},
        {0, 16383, R_HBM, roll_fn<POLICY && N27, NC, 32, 512, 256, 16, WR, PER, true>(), "as above, closed loop"},
        {0, B_ANY, 0, roll_fn<true, NC, 32, 512, 256, 16, WR, PER>(), "the default of this class (comment above)"},
    };
    return run_roll_rules(rules, a, st);
}
// 64 agents: an env is a wave of producers, a row of its observation 3 stores of a writer wave
template <int NC, int PER>
static int launch_roll_64(const Args& a, hipStream_t st) {
    static constexpr RollRule rules[] = {
        {0, 1024, 0, roll_fn<PER == 0, NC, 64, 128, 256, 2, 0, 0>(), "profiles/r04_generic_n.md: a batch that does not fill the chip with 8-env workgroups"},
        {0, B_ANY, 0, roll_fn<true, NC, 64, 512, 256, 8, 0, PER>(), "profiles/r04_generic_n.md"},
    };
    return run_roll_rules(rules, a, st);
}

// The pipelined K-step kernels exist for the agent counts of the reference's hierarchies, N = per^L: the reference's own
// 3^L (README.md:34-36) and the other `per_layer` values get_action_BFS takes (__init__.py:49-56: 2, 4, 5, 8).  per = 0: open
// loop (actions from act_seq); else the closed loop of fg_rollout_hd_policy.  Returns false when (N, per) has no instantiation
// (the caller then runs step_kernel's K-loop / chained launches).
// 3 and 4 agents, open loop, contiguous observations, a batch that fills the chip: one env per lane (fg_hd_lane_kernel.hpp)
template <int NC, int PER = 0, int PW = 1>
static int launch_hd_lane(const Args& a, hipStream_t st) {
    const int grid = 8 * (((a.B + 64 * PW - 1) / (64 * PW) + 7) / 8);
    constexpr int lds = hd_lane_lds_bytes(NC, PW);
    if (describe("hd_lane_kernel<%d,%d,%d> grid %d lds %d; ", NC, PER, PW, grid, lds)) return FG_OK;
    return launch<&hd_lane_kernel<NC, PER, PW>>(grid, 128 * PW, lds, st, "rollout launch failed: %s", a);
}
// One-env-per-lane kernels with four producer waves (256-env workgroups): how full the generations of 256 such workgroups (one per CU) must be - profiles/r05_fill_rule_ab.txt, eleven batch sizes per kernel:
// whole generations or a last one at least three quarters full (a single one: seven eighths: 57344 envs +12 %, 49152 -11 %); `half`:
// a last generation at least half full is enough (basic and formation_hd_env at 3 agents: 98304 envs +5 ... +8 %).
static bool lane_wide_fill(int B, bool half) {
    const int wgs = (B + 255) / 256, full = wgs / 256, rest = wgs % 256;
    return rest == 0 || (full >= 1 && rest >= (half ? 128 : 192)) || (full == 0 && rest >= 224) || full >= 6;
}
// from 32768 envs (512 workgroups of 64 envs: two per CU) the one-env-per-lane kernel wins - 3 x 65536 6.3 -> 3.4 us/step, 4 x 65536
// 9.2 -> 5.0; below, the lane-per-agent kernel spreads a batch over more waves (3 x 16384: 1.62 vs 1.89): profiles/r04_hd_lane_ab.txt
constexpr int FG_HD_LANE_MIN_B = 32768;

static bool launch_pipelined(const Args& a, int per, hipStream_t st, int* rc) {
#define FG_ROLL(FN, NN, PP) if (a.N == NN && per == PP) { *rc = FN<NN, PP>(a, st); return true; }
    if (a.B >= FG_HD_LANE_MIN_B && a.obs_pitch == 3LL * a.N * a.N) {
        // Several producer waves per workgroup - one span of 256 (128) envs per workgroup and step - into a buffer beyond the
        // Infinity Cache (profiles/r05_lane_pw_ab.txt): open loop from 65536 envs with four (3 x 65536 3.02 -> 2.79 us/step, 0.73 ->
        // 0.79 of 8 TB/s in real bytes; 3 x 131072 6.13 -> 5.60, 4 x 131072 10.44 -> 9.61; 4 x 49152 would lose, 3.84 -> 4.47); the
        // closed loop from 98304 envs with two (3 x 98304 5.02 -> 4.28, 4 x 131072 10.18 -> 9.32; at 65536 one stays ahead, 2.70 vs 2.82)
        const double obs_bytes = (double)(a.K / a.obs_every) * a.B * (double)a.obs_pitch * 8.0;
        const bool hbm = obs_bytes > 400e6;
        if (per == 0) {                                 // (3 agents from 260 MB: 3 x 65536 x 20 = 283 MB 3.32 -> 3.06 us/step; 4 agents at 251 MB lose)
            if (a.N == 3 && obs_bytes > 260e6 && lane_wide_fill(a.B, true)) { *rc = launch_hd_lane<3, 0, 4>(a, st); return true; }
            if (a.N == 4 && hbm && lane_wide_fill(a.B, false)) { *rc = launch_hd_lane<4, 0, 4>(a, st); return true; }
        }
        if (hbm && per > 0 && a.B >= 98304) {
            if (a.N == 3 && per == 3) { *rc = launch_hd_lane<3, 3, 2>(a, st); return true; }
            if (a.N == 4 && per == 2) { *rc = launch_hd_lane<4, 2, 2>(a, st); return true; }
        }
        if (a.N == 3 && per == 0) { *rc = launch_hd_lane<3>(a, st); return true; }
        if (a.N == 4 && per == 0) { *rc = launch_hd_lane<4>(a, st); return true; }
        // ... and the closed loop with the controller on the lane's registers (bfs_policy_lane)
        if (a.N == 3 && per == 3) { *rc = launch_hd_lane<3, 3>(a, st); return true; }
        if (a.N == 4 && per == 2) { *rc = launch_hd_lane<4, 2>(a, st); return true; }
        if (a.N == 4 && per == 4) { *rc = launch_hd_lane<4, 4>(a, st); return true; }
    }
    FG_ROLL(launch_roll_8, 3, 0) FG_ROLL(launch_roll_8, 3, 3)
    FG_ROLL(launch_roll_8, 4, 0) FG_ROLL(launch_roll_8, 4, 2) FG_ROLL(launch_roll_8, 4, 4)
    FG_ROLL(launch_roll_8, 8, 0) FG_ROLL(launch_roll_8, 8, 2) FG_ROLL(launch_roll_8, 8, 8)
    FG_ROLL(launch_roll_16, 9, 0) FG_ROLL(launch_roll_16, 9, 3)
    FG_ROLL(launch_roll_16, 16, 0) FG_ROLL(launch_roll_16, 16, 2) FG_ROLL(launch_roll_16, 16, 4)
    FG_ROLL(launch_roll_32, 25, 0) FG_ROLL(launch_roll_32, 25, 5)
    FG_ROLL(launch_roll_32, 27, 0) FG_ROLL(launch_roll_32, 27, 3)
    FG_ROLL(launch_roll_32, 32, 0) FG_ROLL(launch_roll_32, 32, 2)
    FG_ROLL(launch_roll_64, 64, 0) FG_ROLL(launch_roll_64, 64, 2) FG_ROLL(launch_roll_64, 64, 4) FG_ROLL(launch_roll_64, 64, 8)
    // more than 64 agents: the pipelined kernels keep one env on ONE producer wave (~15 / ~78 us of dependent work per step
    // at 81 / 243 agents); a batch too small to hide that under other envs' stores is faster in step_kernel's K-loop, which
    // spreads an env over 2 / 4 waves: 81 x 256 x 20 15.6 -> 12.5 us/step, 81 x 512 18.1 -> 16.1 (81 x 1024: 31.8 vs 33.2, stays),
    // 243 x 64 x 8 77.8 -> 37.0, 243 x 256 81.8 -> 67.8 (243 x 257 on the pipelined kernel: 103; 243 x 512 equal) -
    // profiles/r03_wide/ab_wide_small_kloop.txt.  The closed loop always runs in the pipelined kernel (one launch).
    if (per == 0 && a.B <= 512) return false;
    FG_ROLL(launch_wide, 81, 0) FG_ROLL(launch_wide, 81, 3)
    FG_ROLL(launch_wide, 125, 0) FG_ROLL(launch_wide, 125, 5)
    FG_ROLL(launch_wide, 243, 0) FG_ROLL(launch_wide, 243, 3)
#undef FG_ROLL
    return false;
}

// N = per^L with 2 <= per <= 8: fills the host-rounded constants of the hierarchy
static bool policy_levels_for(int N, int per, FgPolicyLevels* pl) {
    if (per < 2 || per > 8 || N < per) return false;
    memset(pl, 0, sizeof(*pl));
    long long n = 1;
    int L = 0;
    while (n < N && L < FG_POLICY_MAX_LEVELS) { pl->inv_sub[L] = (float)(1.0 / (double)n); n *= per; ++L; }
    if (n != N) return false;
    pl->per = per; pl->L = L; pl->inv_per = (float)(1.0 / (double)per);
    return true;
}

// Args.obs_pitch (float2 units) from FgParams.obs_env_pitch (floats; 0 = contiguous)
static int set_obs_pitch(Args* a) {
    const long long nenv = 6LL * a->N * a->N;
    const long long pitch = a->p.obs_env_pitch ? (long long)a->p.obs_env_pitch : nenv;
    if (pitch < nenv || (pitch & 1))
        return fail(FG_ERR_BAD_ARG, "params: obs_env_pitch must be 0 or an even number of floats >= 6 N^2%s");
    a->obs_pitch = pitch / 2;
    return FG_OK;
}

static int check_params(const FgParams* p) {
    if (!p) return fail(FG_ERR_BAD_ARG, "params is NULL%s");
    if (!(p->mass > 0.f) || !(p->contact_margin > 0.f) || !(p->dt > 0.f))
        return fail(FG_ERR_BAD_ARG, "params: mass, contact_margin and dt must be > 0%s");
    if (p->num_walls < 0 || p->num_walls > FG_MAX_WALLS || p->accel < 0.f || p->max_speed < 0.f || p->u_noise < 0.f)
        return fail(FG_ERR_BAD_ARG, "params: 0 <= num_walls <= 4, accel/max_speed/u_noise >= 0%s");
    if (!(p->dist_min > 0.f)) return fail(FG_ERR_BAD_ARG, "params: dist_min must be > 0%s");
    if (((uintptr_t)p->agent_props & 3u) || ((uintptr_t)p->comm_state & 7u))
        return fail(FG_ERR_ALIGNMENT, "params: agent_props must be 4-byte, comm_state 8-byte aligned%s");
    return FG_OK;
}

// ---- the pieces an entry point builds its call from.  Each check is a function the entry calls at ITS point: the entries do
// not agree on the order (fg_step_hd checks N before it looks at an empty batch, the rollouts after), and the order is ABI.
static int null_pointer(const char* who) { return fail(FG_ERR_BAD_ARG, "%s: a required pointer is NULL", who); }

// the buffers of a K-step formation_hd_env rollout - fg_rollout_hd, fg_rollout_hd_policy and the fused-actor entries - in the
// order in which those entries take them (act_seq: read by fg_rollout_hd, written by the others), and their checks as `who`
struct HdRollout {
    float *pos_x, *pos_y, *vel_x, *vel_y, *act_seq, *ideal_shape, *ideal_vel;
    int32_t* step;
    float *obs_seq, *reward_seq, *indiv_seq;
    uint8_t* done_seq;
};
static int rollout_buffers_check(const char* who, const HdRollout& r) {
    if (!r.pos_x || !r.pos_y || !r.vel_x || !r.vel_y || !r.act_seq || !r.ideal_shape || !r.ideal_vel || !r.step || !r.reward_seq)
        return null_pointer(who);
    if (((uintptr_t)r.obs_seq & 15u) || ((uintptr_t)r.act_seq & 7u) || ((uintptr_t)r.ideal_shape & 7u) || ((uintptr_t)r.ideal_vel & 7u))
        return fail(FG_ERR_ALIGNMENT, "obs_seq must be 16-byte, act_seq/ideal_shape/ideal_vel 8-byte aligned%s");
    return FG_OK;
}

static int policy_levels_check(const char* who, int N, int per, FgPolicyLevels* pl) {
    if (policy_levels_for(N, per, pl)) return FG_OK;
    return fail(FG_ERR_UNSUPPORTED_N, "%s: N must be per_layer^L with 2 <= per_layer <= 8", who);
}

// The start of every formation_hd_env launch description: zeroed, the scalars, the observation pitch (checked).
static int hd_args(Args* a, const FgParams* params, int B, int N, int K, int obs_every, int do_phys, int do_post) {
    memset(a, 0, sizeof(*a));
    a->p = *params; a->B = B; a->N = N; a->inv_n = 1.0f / (float)N; a->K = K; a->obs_every = obs_every < 1 ? 1 : obs_every;
    a->do_phys = do_phys; a->do_post = do_post;
    return set_obs_pitch(a);
}
// ... and its state and output buffers (the actions, a.act or a.act_out, and the index outputs are the entry's own)
static void hd_buffers(Args* a, float* px, float* py, float* vx, float* vy, float* shape, float* ivel, int32_t* step,
                       float* obs, float* rew, float* indiv, uint8_t* done) {
    a->px = px; a->py = py; a->vx = vx; a->vy = vy; a->shape = shape; a->ivel = ivel; a->step = step;
    a->obs = obs; a->rew = rew; a->indiv = indiv; a->done = done;
}
static void hd_buffers(Args* a, const HdRollout& r) {
    hd_buffers(a, r.pos_x, r.pos_y, r.vel_x, r.vel_y, r.ideal_shape, r.ideal_vel, r.step, r.obs_seq, r.reward_seq, r.indiv_seq, r.done_seq);
}

// ---- the reference's demo controller (fg_policy_kernels.hpp): one launch geometry and one PER switch for both of its kernels
struct PolicyGeometry { int lpe, grid, lds; };                         // lpe lanes per env, 256 threads per workgroup
static PolicyGeometry policy_geometry(int B, int N) {
    const int lpe = N <= 16 ? 16 : N <= 32 ? 32 : N <= 64 ? 64 : 256;
    const int E = 256 / lpe;
    return {lpe, (B + E - 1) / E, E * policy_block_units(N) * (int)sizeof(float2)};     // lds <= 56 KiB
}
template <class F>
static int policy_per_dispatch(int per, F&& run) {                     // run(per) with `per` as the `value` of the argument's type
#define FG_POLICY(PER) case PER: return run(IntC<PER>{});
    switch (per) { FG_POLICY(2) FG_POLICY(3) FG_POLICY(4) FG_POLICY(5) FG_POLICY(6) FG_POLICY(7) FG_POLICY(8) }
#undef FG_POLICY
    return FG_OK;                                                      // (policy_levels_for admits 2 ... 8 only)
}
// the controller from the simulator state: one launch, shared by fg_policy_bfs_state and the chained closed loop
static int launch_policy_state(int B, int N, const FgPolicyLevels& pl, const float* px, const float* py,
                               const float* shape, const float* ivel, float* act, hipStream_t st) {
    const PolicyGeometry g = policy_geometry(B, N);
    if (describe("policy_state_kernel<%d> grid %d lds %d; ", pl.per, g.grid, g.lds)) return FG_OK;
    return policy_per_dispatch(pl.per, [&](auto per) {
        return launch<&policy_state_kernel<decltype(per)::value>>(g.grid, 256, g.lds, st, "policy launch failed: %s", B, N, g.lpe,
                                                                  pl, px, py, shape, ivel, act);
    });
}

// one env per lane, PW producer waves (64 PW envs) and PW * scn_lane_writers(KIND) writer waves per workgroup
// Four producer waves - 256 envs, one span of 55 ... 133 KB per workgroup and step instead of four - where such workgroups
// come in whole generations of 256 (one per CU; or in six generations and more) - profiles/r05_lane_pw_ab.txt:
//   basic 3 x 65536 3.04 -> 2.83 us/step (0.72 -> 0.77 of 8 TB/s, all bytes), 3 x 131072 6.26 -> 5.67 (0.70 -> 0.77);
//   partial 5 x 131072 12.85 -> 12.51, range 4 x 131072 10.20 -> 9.33 (equal or slower at 65536: 6.44 / 6.40, 4.60 / 4.80);
//   obstacle never (5.47 / 5.65, 11.25 / 11.24); half-filled generations lose everywhere (32768 envs: 1.70 -> 2.40).
// Measured on rollouts whose observation buffer does not fit the Infinity Cache (> 260 MB: R_BEYOND_IC of the formation_hd_env rules): only those.
template <int KIND> static bool scn_lane_wide(int B, double obs_bytes) {
    if (obs_bytes <= 260e6) return false;
    if (KIND == FG_SCN_BASIC) return lane_wide_fill(B, true);
    // partial / range: whole generations from the second on only - on boxes whose placed buffers run fast the 256-env form loses 1-5 % at
    // 57344 / 65536 / 114688 envs (it wins 7-13 % there on slow compositions and ordinary allocations), at 131072 it wins on both
    const int wgs = (B + 255) / 256;
    return (KIND == FG_SCN_PARTIAL || KIND == FG_SCN_RANGE) && B >= 131072 && (wgs % 256 == 0 || wgs >= 6 * 256);
}
template <int KIND, int NN, int LL, int MM, int NBR, int PW>
static int launch_scn_lane(const ScnArgs& a, hipStream_t st) {
    constexpr int lds = scn_lane_lds_bytes(KIND, NN, LL, MM, NBR, PW);
    constexpr int threads = 64 * PW * (1 + scn_lane_writers(KIND));
    const int grid = 8 * (((a.B + 64 * PW - 1) / (64 * PW) + 7) / 8);
    if (describe("scn_lane_kernel<%d,%d,%d,%d,%d,%d> grid %d threads %d lds %d; ", KIND, NN, LL, MM, NBR, PW, grid, threads, lds)) return FG_OK;
    return launch<&scn_lane_kernel<KIND, NN, LL, MM, NBR, PW>>(grid, threads, lds, st, "scenario launch failed: %s", a);
}
// The reference's own scenario shapes, every count a compile-time constant (fg_scn_lane_kernel.hpp, fg_scn_lane_actor_kernel.hpp):
// X(kind, agents, landmarks, obstacles, neighbours an agent sees, WIDE).  WIDE: the 256-env form of the lane kernel exists for
// this shape (scn_lane_wide); the fused-actor kernels have no such form.
#define FG_SCN_SHAPES(X)                                                                                                 \
    X(FG_SCN_BASIC, 3, 3, 0, 2, true)            /* basic_formation_env.py:7 */                                             \
    X(FG_SCN_PARTIAL, 5, 5, 0, 3, true)          /* formation_hd_partial_env.py:15 */                                       \
    X(FG_SCN_RANGE, 4, 4, 0, 3, true)            /* formation_hd_partial_range_env.py:15 */                                 \
    X(FG_SCN_OBSTACLE, 4, 4, 3, 3, false)        /* formation_hd_obs_env.py:14 */                                           \
    X(FG_SCN_PARTIAL, 3, 5, 0, 3, false)         /* make_env(name) passes its own default num_agents = 3 (__init__.py:6-11) */ \
    X(FG_SCN_RANGE, 3, 4, 0, 2, false)                                                                                   \
    X(FG_SCN_OBSTACLE, 3, 4, 3, 2, false)

}  // namespace fg

using namespace fg;

// ---------------------------------------------------------------------------
// What the entry points below are made of: an entry checks its call, builds the launch description (hd_args / scn_args and
// the buffers) and hands it to a dispatch; the dispatches are also walked dry by the fg_describe_* entries.
// ---------------------------------------------------------------------------

// fg_step_hd in two halves: argument checks + the launch description, and the dispatch of a checked description
static int step_hd_describe(const FgParams* params, int B, int N,
                            float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                            const float* act, float* ideal_shape, float* ideal_vel, int32_t* step,
                            float* obs, float* reward, float* indiv_reward, uint8_t* done,
                            int32_t* near_lm, int32_t* near_ag, int32_t* hd_idx, Args* a) {
    int rc = check_params(params);
    if (rc) return rc;
    if (B < 0) return fail(FG_ERR_BAD_ARG, "B must be >= 0%s");
    if ((rc = hd_n_check(N))) return rc;
    if (B > 0 && (!pos_x || !pos_y || !vel_x || !vel_y || !act || !ideal_shape || !ideal_vel || !step || !obs || !reward))
        return null_pointer("fg_step_hd");
    if (((uintptr_t)obs & 15u) || ((uintptr_t)act & 7u) || ((uintptr_t)ideal_shape & 7u) || ((uintptr_t)ideal_vel & 7u))
        return fail(FG_ERR_ALIGNMENT, "obs must be 16-byte, act/ideal_shape/ideal_vel 8-byte aligned%s");
    if ((rc = hd_args(a, params, B, N, 1, 1, 1, 1))) return rc;
    hd_buffers(a, pos_x, pos_y, vel_x, vel_y, ideal_shape, ideal_vel, step, obs, reward, indiv_reward, done);
    a->act = act; a->near_lm = near_lm; a->near_ag = near_ag; a->hd_idx = hd_idx;
    return FG_OK;
}

static int step_hd_dispatch(const Args& a, hipStream_t stream) {
    if (a.B == 0) return FG_OK;                       // an empty batch is a no-op (e.g. a rank that owns no envs)
    const bool plain = !world_options_set(a.p) && !a.near_lm && !a.near_ag && !a.hd_idx;
    // 243 agents, >= 4096 envs: pipeline over env batches inside the launch (no index outputs, no World options):
    // 1.85-2.2 ms vs 2.1-2.3 ms at 243 x 8192 (round 1; 1.75 ms on placed buffers).
    if (a.N == 243 && a.B >= FG_WIDE243_MIN_B && plain) return launch_wide<243, 0>(a, stream);
    // 81 agents: the pipelined kernel pays from 16 env batches per workgroup on (81 x 16384: 419 vs 448 us; 81 x 12288 equal,
    // 81 x 2048 62 vs 56: profiles/r03_step/pipelined_single_step_81.txt)
    if (a.N == 81 && a.B >= FG_WIDE81_MIN_B && plain) return launch_wide<81, 0>(a, stream);
    return launch_step(a, stream);
}

// A step loop that re-uses its buffers launches the same description again and again with only the RNG offset moving: the
// plan keeps the checked description, so the per-step host work is one two-argument call and the kernel launch (a ctypes
// call with 19 arguments cost 1.7 us per env.step on top of the 7.7 us kernel at 9 x 4096: VERDICT r4).
namespace { struct StepPlan { Args a; hipStream_t stream; int device; }; }

// the tail of fg_rollout_hd: which kernel runs a checked K-step description (also walked dry by fg_describe_launch)
static int rollout_hd_dispatch(const Args& a, hipStream_t st) {
    int rc = FG_OK;
    // K >= 2 at the specialised agent counts: producer / writer pipelined kernels.  World options (walls, max_speed,
    // accel, u_noise) exist only in step_kernel's OPTS instantiation, whose K-loop runs the rollout then.
    if (a.K == 1 && !world_options_set(a.p)) {                                                       // as fg_step_hd
        if (a.N == 243 && a.B >= FG_WIDE243_MIN_B) return launch_wide<243, 0>(a, st);
        if (a.N == 81 && a.B >= FG_WIDE81_MIN_B) return launch_wide<81, 0>(a, st);
    }
    if (a.K >= 2 && !world_options_set(a.p) && launch_pipelined(a, 0, st, &rc)) return rc;
    return launch_step(a, st);
}

// ... and of fg_rollout_hd_policy (a.pl, a.act_out set)
static int rollout_hd_policy_dispatch(const Args& a, int per_layer, hipStream_t st) {
    int rc = FG_OK;
    // N = per^L up to 243 agents (per 2, 3, 4, 5, 8): the controller runs inside the pipelined kernels, ONE launch
    if (!world_options_set(a.p) && launch_pipelined(a, per_layer, st, &rc)) return rc;
    // everything else: K times (controller launch, single-step launch) chained on the stream - the same device
    // function on the same state, so the results equal the in-kernel loop's and fg_policy_bfs on the written rows
    const size_t bn = (size_t)a.B * a.N;
    for (int k = 0; k < a.K; ++k) {
        float* act_k = a.act_out + (size_t)k * bn * 2;
        rc = launch_policy_state(a.B, a.N, a.pl, a.px, a.py, a.shape, a.ivel, act_k, st);
        if (rc) return rc;
        Args s1 = a;
        s1.K = 1; s1.obs_every = 1; s1.act = act_k; s1.act_out = nullptr;
        s1.p.rng_offset = a.p.rng_offset + (uint64_t)k;
        s1.rew = a.rew + (size_t)k * bn;
        s1.indiv = a.indiv ? a.indiv + (size_t)k * bn : nullptr;
        s1.done = a.done ? a.done + (size_t)k * bn : nullptr;
        s1.obs = (a.obs && (k + 1) % a.obs_every == 0)
                     ? a.obs + (size_t)(k / a.obs_every) * (size_t)a.B * (size_t)a.obs_pitch * 2 : nullptr;
        rc = launch_step(s1, st);
        if (rc) return rc;
        if (g_describe && k == 0 && a.K > 1) { describe("x %d chained; ", a.K); break; }   // dry run: one round says it all
    }
    return FG_OK;
}

// ---- 16-bit observations out of the rollout launch (fg_rollout_hd_obs16, fg_rollout_hd_policy_obs16) ----
// A dispatch of its own, reached only from those entries and their dry run: ONE instantiation per (agents, loop, format) with the
// geometry of the fp32 default of its class (the last rule of launch_roll_8 / _16 / _32) and the 16-bit writer of
// fg_obs_writers.hpp as WR.  The fp32 rule tables above never name these kernels.
template <int WR>
static int obs16_launch(const Args& a, int per, hipStream_t st) {
#define FG_OBS16(NN, G, TP, TW, E)                                                                               \
    if (a.N == NN) {                                                                                             \
        static_assert(roll_lds_bytes<NN, TW, E, WR, 3>() <= 160 * 1024, "16-bit rollout LDS");                  \
        return per ? launch_roll_v<NN, G, TP, TW, E, WR, 3>(a, st) : launch_roll_v<NN, G, TP, TW, E, WR, 0>(a, st); \
    }
    FG_OBS16(27, 32, 512, 256, 16) FG_OBS16(9, 16, 64, 128, 4) FG_OBS16(3, 4, 64, 128, 16)
#undef FG_OBS16
    return fail(FG_ERR_UNSUPPORTED_N, "16-bit observations: no fused launch for this agent count%s");   // (unreachable after obs16_check)
}
static int obs16_dispatch(const Args& a, int obs_format, int per, hipStream_t st) {
    return obs_format == FG_OBS_F16 ? obs16_launch<FG_WR_OBS_F16>(a, per, st) : obs16_launch<FG_WR_OBS_BF16>(a, per, st);
}
// The checks the two entries and their dry run share, before the buffers: FG_OK, or the status of the first that fails.
// per_layer 0: open loop; `pl` receives the controller's constants otherwise.
static int obs16_check(const char* who, const FgParams* params, int obs_format, int B, int N, int K, int per_layer, FgPolicyLevels* pl) {
    if (const int rc = check_params(params)) return rc;
    if (obs_format != FG_OBS_F16 && obs_format != FG_OBS_BF16) return fail(FG_ERR_BAD_ARG, "%s: obs_format must be FG_OBS_F16 or FG_OBS_BF16", who);
    if (B < 0 || K < 2) return fail(FG_ERR_BAD_ARG, "%s: B >= 0 and K >= 2 required", who);
    if (world_options_set(*params))
        return fail(FG_ERR_BAD_ARG, "%s: World options (walls, noise, max_speed, accel, agent_props, comm_state) have no 16-bit launch", who);
    if (params->obs_env_pitch != 0) return fail(FG_ERR_BAD_ARG, "%s: a padded env pitch (obs_env_pitch) is not supported", who);
    if (N != 3 && N != 9 && N != 27) return fail(FG_ERR_UNSUPPORTED_N, "%s: N must be 3, 9 or 27", who);
    if (per_layer != 0 && (per_layer != 3 || !policy_levels_for(N, per_layer, pl)))
        return fail(FG_ERR_UNSUPPORTED_N, "%s: the closed loop needs per_layer = 3", who);
    return FG_OK;
}
// ... and the rest of an entry: buffers, launch description (fg_rollout_hd's builder), dispatch.  r.obs_seq holds 32-bit units.
static int obs16_rollout(const char* who, const FgParams* params, int obs_format, int B, int N, int K, int per_layer,
                         const HdRollout& r, int obs_every, void* stream) {
    FgPolicyLevels pl;
    int rc = obs16_check(who, params, obs_format, B, N, K, per_layer, &pl);
    if (rc) return rc;
    if (B == 0) return FG_OK;                         // an empty batch is a no-op (e.g. a rank that owns no envs)
    if (obs_every < 1) return fail(FG_ERR_BAD_ARG, "%s: obs_every >= 1 required", who);
    if (!r.obs_seq) return null_pointer(who);
    if ((rc = rollout_buffers_check(who, r))) return rc;
    const DeviceGuard device_guard(stream, r.pos_x);
    Args a;
    if ((rc = hd_args(&a, params, B, N, K, obs_every, 1, 1))) return rc;
    hd_buffers(&a, r);
    if (per_layer) { a.pl = pl; a.act_out = r.act_seq; } else a.act = r.act_seq;
    return obs16_dispatch(a, obs_format, per_layer, (hipStream_t)stream);
}

static int launch_mt_reset(int B, int N, const uint8_t* mask, uint32_t* mt_state,
                           float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                           float* ideal_shape, float* ideal_vel, float* landmark_pos, int32_t* step,
                           int world_length, float* obs, long long obs_env_pitch, void* stream) {
    const DeviceGuard device_guard(stream, pos_x);
    if (B == 0) return FG_OK;                         // an empty batch is a no-op (e.g. a rank that owns no envs)
    if (B < 0) return fail(FG_ERR_BAD_ARG, "B must be >= 0%s");
    if (const int rc = generic_n_check(N)) return rc;
    if (!mt_state || !pos_x || !pos_y || !vel_x || !vel_y || !ideal_shape || !ideal_vel) return null_pointer("fg_reset_hd_mt");
    const long long nenv = 6LL * N * N;
    const long long pitch = obs_env_pitch ? obs_env_pitch : nenv;
    if (obs && (pitch < nenv || (pitch & 1))) return fail(FG_ERR_BAD_ARG, "obs_env_pitch must be 0 or an even number of floats >= 6 N^2%s");
    if ((uintptr_t)obs & 7u) return fail(FG_ERR_ALIGNMENT, "obs must be 8-byte aligned%s");
    const int lds = (624 + ((8 * N + 4 + 1) & ~1)) * (int)sizeof(uint32_t) + 2 * (int)sizeof(double) +
                    (2 * N + 1) * (int)sizeof(float2);
    return launch<&mt_reset_kernel>(B, 256, lds, (hipStream_t)stream, "mt reset launch failed: %s", B, N, mask, mt_state, pos_x, pos_y,
                                    vel_x, vel_y, ideal_shape, ideal_vel, landmark_pos, step, world_length, obs, pitch / 2);
}

// ---- the landmark scenarios: the checks the step / rollout entries and the two resets share, each called at the entry's own
// point (the resets name themselves in their pointer check and do not look at the buffers the step needs)
constexpr int FG_NOOP = 1;         // a check's answer to zero steps or an empty batch: the entry returns FG_OK without a launch
static int scn_given(const FgScenario* sc) { return sc ? FG_OK : fail(FG_ERR_BAD_ARG, "scenario descriptor is NULL%s"); }
static int scn_kind_check(const FgScenario* sc) {
    return sc->kind < FG_SCN_BASIC || sc->kind > FG_SCN_OBSTACLE ? fail(FG_ERR_BAD_ARG, "unknown scenario kind%s") : FG_OK;
}
static int scn_counts_check(const FgScenario* sc, int B, int N) {
    const int L = sc->num_landmarks, M = sc->num_obstacles;
    if (B < 0 || L <= 0 || M < 0) return fail(FG_ERR_BAD_ARG, "B >= 0, L > 0, M >= 0 required%s");
    if (N < 2 || N + M > FG_MAX_AGENTS || L > 1024)
        return fail(FG_ERR_UNSUPPORTED_N, "scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024%s");
    return FG_OK;
}
// a NULL among the world's buffers (the obstacles' only where the scenario has any)
static bool scn_world_null(const FgScenario* sc, const float* px, const float* py, const float* vx, const float* vy,
                           const float* landmarks, const float* obst_pos, const float* obst_vel) {
    return !px || !py || !vx || !vy || !landmarks || (sc->num_obstacles > 0 && (!obst_pos || !obst_vel));
}
static int scn_reset_align_check(const float* landmarks, const float* obst_pos, const float* obst_vel) {
    if (((uintptr_t)landmarks & 7u) || ((uintptr_t)obst_pos & 7u) || ((uintptr_t)obst_vel & 7u))
        return fail(FG_ERR_ALIGNMENT, "landmarks / obstacle buffers must be 8-byte aligned%s");
    return FG_OK;
}

// The scalars of a landmark-scenario launch description (the fused-actor entries come here with a descriptor whose landmark
// count nobody has checked yet: their dispatch refuses every shape but the reference's).
static void scn_args(ScnArgs* a, const FgParams* params, const FgScenario* sc, int B, int N, int do_physics, int K, int obs_every) {
    a->p = *params; a->sc = *sc; a->B = B; a->N = N; a->do_phys = do_physics ? 1 : 0; a->K = K; a->obs_every = obs_every < 1 ? 1 : obs_every;
    a->inv_n = (float)(1.0 / (double)N); a->inv_l = (float)(1.0 / (double)(sc->num_landmarks > 0 ? sc->num_landmarks : 1));
    a->coll_scale = (float)((double)params->collide_thresh / (double)params->dist_min);
}
// ... and its buffers: a zeroed description with the caller's pointers in it
static ScnArgs scn_buffers(float* px, float* py, float* vx, float* vy, const float* act, float* landmarks, float* obst_pos,
                           float* obst_vel, int32_t* step, float* obs, float* rew, float* indiv, uint8_t* done, int32_t* near_ag) {
    ScnArgs a; memset(&a, 0, sizeof(a));
    a.px = px; a.py = py; a.vx = vx; a.vy = vy; a.act = act; a.lm = landmarks; a.opos = obst_pos; a.ovel = obst_vel; a.step = step;
    a.obs = obs; a.rew = rew; a.indiv = indiv; a.done = done; a.near_ag = near_ag;
    return a;
}

// The checks of a step / rollout of a landmark scenario before its buffers: FG_OK, FG_NOOP, or the status of the first that fails
static int scenario_check(const FgParams* params, const FgScenario* sc, int B, int N, int do_physics, int K, int obs_every) {
    int rc = check_params(params);
    if (rc || (rc = scn_given(sc))) return rc;
    if (K == 0) return FG_NOOP;
    if (K < 0 || obs_every < 1) return fail(FG_ERR_BAD_ARG, "K >= 0 and obs_every >= 1 required%s");
    if (K > 1 && !do_physics) return fail(FG_ERR_BAD_ARG, "a multi-step launch steps the physics%s");
    if (params->comm_state)
        return fail(FG_ERR_BAD_ARG, "comm_state is honoured by the formation_hd_env entry points only%s");
    if ((rc = scn_kind_check(sc))) return rc;
    if (B == 0) return FG_NOOP;
    if ((rc = scn_counts_check(sc, B, N))) return rc;
    if (sc->kind == FG_SCN_PARTIAL && (sc->num_obs < 0 || sc->num_obs > 1024)) return fail(FG_ERR_BAD_ARG, "bad num_obs%s");
    return FG_OK;
}

// which kernel runs a checked description (also walked dry by fg_describe_launch)
static int scenario_dispatch(ScnArgs a, hipStream_t st) {
    const int B = a.B, N = a.N, L = a.sc.num_landmarks, M = a.sc.num_obstacles;
    const int nbr = a.sc.kind == FG_SCN_PARTIAL ? a.sc.num_obs : N - 1;
    if (a.sc.variant != 1 && !a.p.agent_props) {           // (per-agent tables: the run-time-count kernel)
        // the reference's own shapes: one env per lane, every count a compile-time constant (fg_scn_lane_kernel.hpp)
        const double obs_bytes = (double)(a.K / a.obs_every) * B * N * 4.0 * scn_obs_dim(a.sc.kind, N, L, M, nbr);
#define FG_SCN_LANE(KIND, NN, LL, MM, NBR, WIDE)                                                         \
        if (a.sc.kind == KIND && N == NN && L == LL && M == MM && nbr == NBR)                            \
            return WIDE && scn_lane_wide<KIND>(B, obs_bytes) ? launch_scn_lane<KIND, NN, LL, MM, NBR, (WIDE ? 4 : 1)>(a, st) \
                                                             : launch_scn_lane<KIND, NN, LL, MM, NBR, 1>(a, st);
        FG_SCN_SHAPES(FG_SCN_LANE)
#undef FG_SCN_LANE
    }
    const int G = scn_group_lanes(N + M);
    const int E = scn_envs_per_group(G);              // more than 64 entities: one env per workgroup of G threads
    const int grid = (B + E - 1) / E;
    int lds = (int)scn_lds_bytes(G, N, L, M, 0);
    {   // observation rows composed in LDS and streamed out contiguously when the workgroup's block fits
        const long long staged = scn_lds_bytes(G, N, L, M, scn_obs_dim(a.sc.kind, N, L, M, nbr));
        a.stage = (staged <= 48 * 1024) ? 1 : 0;
        if (a.stage) lds = (int)staged;
    }
    if (describe("scn_kernel<%d,%d> grid %d lds %d stage %d; ", G, G <= 64 ? FG_SCN_T : G, grid, lds, a.stage)) return FG_OK;
    return pow2_dispatch(G, [&](auto g, auto t) {
        return launch<&scn_kernel<decltype(g)::value, decltype(t)::value>>(grid, decltype(t)::value, lds, st, "scenario launch failed: %s", a);
    });
}

// fg_step_scenario, fg_step_basic and fg_rollout_scenario: `a` holds the caller's buffers (scn_buffers)
static int launch_scenario(const FgParams* params, const FgScenario* sc, int B, int N, int do_physics, int K, int obs_every,
                           ScnArgs a, void* stream) {
    const DeviceGuard device_guard(stream, a.px);
    const int rc = scenario_check(params, sc, B, N, do_physics, K, obs_every);
    if (rc) return rc == FG_NOOP ? FG_OK : rc;
    if (scn_world_null(sc, a.px, a.py, a.vx, a.vy, a.lm, a.opos, a.ovel) || !a.obs || (do_physics && (!a.act || !a.rew)))
        return null_pointer("scenario step");
    if (((uintptr_t)a.obs & 7u) || ((uintptr_t)a.lm & 7u) || (a.act && ((uintptr_t)a.act & 7u)) ||
        ((uintptr_t)a.opos & 7u) || ((uintptr_t)a.ovel & 7u))
        return fail(FG_ERR_ALIGNMENT, "obs/landmarks/act/obstacle buffers must be 8-byte aligned%s");
    scn_args(&a, params, sc, B, N, do_physics, K, obs_every);
    return scenario_dispatch(a, (hipStream_t)stream);
}

// ---- closed loop with the caller's MLP actor (fg_actor_rollout_kernel.hpp) ----
static bool actor_n_supported(int N) {
    return N == 3 || N == 4 || N == 8 || N == 9 || N == 16 || N == 25 || N == 27 || N == 32;
}
// Describe-or-launch of an actor kernel: Det (the deterministic actor; log_std == NULL) or its sampling twin Smp (the Gaussian
// actor), which takes (log_std, logp) after Det's arguments `args`.  `targs` spells the template arguments and `unit` the word
// before the thread count in the describe string; `lds` is the chosen kernel's.
template <auto Det, auto Smp, class... A>
static int launch_actor_pair(const char* det_name, const char* smp_name, const char* targs, const char* unit, int grid,
                             int threads, int envs, int lds, const char* fail_fmt, hipStream_t st, const float* log_std,
                             float* logp, const A&... args) {
    const bool sample = log_std != nullptr;
    if (describe("%s<%s> grid %d %s %d envs/wg %d lds %d; ", sample ? smp_name : det_name, targs, grid, unit, threads, envs, lds))
        return FG_OK;
    if (sample) return launch<Smp>(grid, threads, lds, st, fail_fmt, args..., log_std, logp);
    return launch<Det>(grid, threads, lds, st, fail_fmt, args...);
}

// The formation_hd_env actor families: HdActorFamily<kind> (fg_actor_rollout_kernel.hpp) holds each family's flags, widest H,
// members and failure text; here are the entry point that names each kind and the kernels' operands after `a` (hd_actor_dispatch):
//     HD_ACTOR_SHARED        ActorW                          HD_ACTOR_GRU           ActorW, ActorNormW, ActorGruW
//     HD_ACTOR_PER_AGENT     ActorTab                        HD_ACTOR_BN            ActorW, ActorBnW
//     HD_ACTOR_NORM          ActorW, ActorNormW              HD_ACTOR_BN_PER_AGENT  ActorTab, ActorBnTab
static const char* const hd_actor_entry[] = {"fg_rollout_hd_actor", "fg_rollout_hd_actor_sample", "fg_rollout_hd_actor_per_agent",
                                             "fg_rollout_hd_actor_norm", "fg_rollout_hd_actor_gru", "fg_rollout_hd_actor_bn",
                                             "fg_rollout_hd_actor_bn_per_agent"};

// Describe-or-launch of the member M of the family F at <NC, H>: `args` are the kernel's arguments after `a` - the family's
// operands, then the member's.  The LDS bytes come from the value the kernel's own flags come from.
template <ActorMember M, int NC, int H, class F, class... A>
static int launch_hd_member(const Args& a, hipStream_t st, const A&... args) {
    if constexpr (F::has(M, NC, H)) {
        constexpr int E = actor_envs(NC), lds = actor_lds_bytes(NC, H, F::flags, M);
        static_assert(lds <= 160 * 1024, "actor rollout LDS");
        const int grid = (a.B + E - 1) / E;
        if (describe("%s<%d,%d> grid %d block %d envs/wg %d lds %d; ", F::name(M), NC, H, grid, FG_ACTOR_THREADS, E, lds)) return FG_OK;
        return launch<F::template kernel<M, NC, H>()>(grid, FG_ACTOR_THREADS, lds, st, F::fail_fmt, a, args...);
    } else {                                           // (no entry builds such a call: hd_actor_check)
        return actor_member_obs16(M) ? fail(FG_ERR_UNSUPPORTED_N, "16-bit observations: no fused actor launch for this family, agent count or width%s")
                                     : fail(FG_ERR_BAD_ARG, "this actor family has no such member%s");
    }
}

// A failed check of an actor description, in the name of the entry `who` [and of the per-agent entry's member `member`]:
// "<who>: [member <i>: ]<what, with arg>" as the error text, `code` as the status.
struct ActorComplaint {
    const char* who;
    int member = -1;
    int operator()(int code, const char* what, const char* arg = "") const {
        char text[128], idx[24] = "", msg[192];
        snprintf(text, sizeof(text), what, arg);
        if (member >= 0) snprintf(idx, sizeof(idx), "member %d: ", member);
        snprintf(msg, sizeof(msg), "%s: %s%s", who, idx, text);
        return fail(code, "%s", msg);
    }
};
static bool actor_eps_ok(float e) { return e > 0.0f && std::isfinite(e); }

// The checks of one FgActor (no device touched): FG_OK, or the status of the first one that fails.  `who` is the entry point
// the messages name, `max_hidden` / `widths` its admissible hidden widths (32, 64 and up to max_hidden), `also` further
// pointers that share the weights' 4-byte alignment check and `aligned` what the alignment message calls them all.
static int actor_struct_check(const FgActor* actor, const char* who, int max_hidden, const char* widths, uintptr_t also,
                              const char* aligned) {
    const ActorComplaint bad{who};
    if (!actor) return bad(FG_ERR_BAD_ARG, "actor is NULL");
    if (actor->hidden != 32 && actor->hidden != 64 && !(actor->hidden == 128 && max_hidden == 128))
        return bad(FG_ERR_BAD_ARG, "hidden must be %s", widths);
    if (!actor->w1 || !actor->w2 || !actor->w3) return bad(FG_ERR_BAD_ARG, "a weight pointer is NULL");
    if (((uintptr_t)actor->w1 | (uintptr_t)actor->w2 | (uintptr_t)actor->w3 | (uintptr_t)actor->b1 | (uintptr_t)actor->b2 |
         (uintptr_t)actor->b3 | also) & 3u)
        return bad(FG_ERR_ALIGNMENT, "%s must be 4-byte aligned", aligned);
    return FG_OK;
}
static int hd_actor_struct_check(const FgParams* params, const FgActor* actor) {
    const int rc = actor_struct_check(actor, "fg_rollout_hd_actor", 128, "32, 64 or 128", 0, "weights");
    if (rc) return rc;
    if (world_options_set(*params))
        return fail(FG_ERR_BAD_ARG, "fg_rollout_hd_actor: World options, per-agent properties and communication are not supported%s");
    return FG_OK;
}

// One call of a formation_hd_env actor entry, fg_rollout_hd_actor* or its fg_describe_actor*_launch twin, as its checks
// (hd_actor_check) and its dispatch (hd_actor_dispatch) take it; the fields in the order in which the kinds add them, so that
// every entry is one brace initialiser.  `actor`: the one shared actor, or for the per-agent kinds a host array of N members;
// `log_std` NULL: the deterministic actor (HD_ACTOR_SAMPLE requires it); `logp`: the log-densities' destination, NULL from a
// describe twin; `in_bn` (HD_ACTOR_BN: the one input BatchNorm; HD_ACTOR_BN_PER_AGENT: a host array of N); `norm` counts for
// HD_ACTOR_NORM and HD_ACTOR_GRU only; `gru` and `rnn_state` (HD_ACTOR_GRU only): the recurrent layer and the hidden state
// [B][N][H], a stand-in address from a describe twin; `noise`: the OU entries' parameters and state, likewise.
struct HdActorNoise {                                  // fg_rollout_hd_actor_ou*: the OU parameters and the noise state [B][N][2]
    bool on = false;
    const FgActorOu* ou = nullptr;
    float* state = nullptr;
};
struct HdActorHead {                                   // fg_rollout_hd_actor_cat: the categorical head's facts and its outputs [K][B][N]
    bool on = false;
    int mode = 0, greedy = 0;
    int32_t* idx = nullptr;
    float* logp = nullptr;
};
struct HdActorGumbel {                                 // fg_rollout_hd_actor_gumbel*: the Gumbel head's facts and its output [K][B][N]
    bool on = false;
    int mode = 0, explore = 0;
    int32_t* idx = nullptr;
};
struct HdActorCall {
    HdActorKind kind;
    const FgActor* actor;
    const float* log_std = nullptr;
    float* logp = nullptr;
    const FgActorInBn* in_bn = nullptr;
    const FgActorNorm* norm = nullptr;
    const FgActorGru* gru = nullptr;
    float* rnn_state = nullptr;
    // fg_rollout_hd_actor_gru_states only (`states_entry`, which also puts its name on the recurrent entry's messages): the
    // record of the states [ceil(K / states_every)][B][N][H]
    bool states_entry = false;
    float* rnn_states = nullptr;
    int states_every = 1;
    // fg_rollout_hd_actor_ou and fg_rollout_hd_actor_ou_per_agent only (`noise.on`, which also puts their names on the messages):
    // the kind is the inner actor's family - shared or per-agent, with `in_bn` the BatchNorm one - whose OU member runs
    HdActorNoise noise = {};
    // fg_rollout_hd_actor_cat only (`cat.on`, which also puts its name on the messages): the kind is the body's family - shared,
    // LayerNorm or recurrent - whose categorical member runs
    HdActorHead cat = {};
    // fg_rollout_hd_actor_obs16 and fg_rollout_hd_actor_cat_obs16 only (not 0, which also puts their names on the messages):
    // FG_OBS_F16 / FG_OBS_BF16, or -1 for a value that is neither; the kind is the body's family, whose 16-bit Gaussian or
    // - `cat.on` - categorical member runs, and the observations' buffer holds 16-bit elements
    int obs_format = 0;
    // fg_rollout_hd_actor_gumbel and fg_rollout_hd_actor_gumbel_per_agent only (`gumbel.on`, which also puts their names on the
    // messages): the kind is the logits' family - shared or per-agent, with `in_bn` the BatchNorm one - whose Gumbel member runs
    HdActorGumbel gumbel = {};
};
static bool hd_actor_members(const HdActorCall& c) { return c.kind == HD_ACTOR_PER_AGENT || c.kind == HD_ACTOR_BN_PER_AGENT; }
// the member of the call's family that runs: the one place that reads these five fields for it
static ActorMember hd_actor_member(const HdActorCall& c) {
    if (c.gumbel.on) return ACTOR_GUMBEL;
    if (c.obs_format) return c.cat.on ? ACTOR_CAT16 : ACTOR_GAUSS16;
    if (c.cat.on) return ACTOR_CAT;
    if (c.noise.on) return ACTOR_OU;
    return c.log_std ? ACTOR_GAUSS : ACTOR_DET;
}
static const char* hd_actor_who(const HdActorCall& c) {
    switch (hd_actor_member(c)) {
    case ACTOR_CAT16: return "fg_rollout_hd_actor_cat_obs16";
    case ACTOR_GAUSS16: return "fg_rollout_hd_actor_obs16";
    case ACTOR_CAT: return "fg_rollout_hd_actor_cat";
    case ACTOR_OU: return hd_actor_members(c) ? "fg_rollout_hd_actor_ou_per_agent" : "fg_rollout_hd_actor_ou";
    case ACTOR_GUMBEL: return hd_actor_members(c) ? "fg_rollout_hd_actor_gumbel_per_agent" : "fg_rollout_hd_actor_gumbel";
    default: return c.states_entry ? "fg_rollout_hd_actor_gru_states" : hd_actor_entry[c.kind];
    }
}
// FgActorNorm's checks (no device touched), in the name of the entry `who`: hidden 32 or 64, every eps that is read positive and
// finite, gamma / beta 4-byte aligned
static int actor_norm_check(const char* who, const FgActor* actor, const FgActorNorm* norm) {
    const ActorComplaint bad{who};
    if (!norm) return bad(FG_ERR_BAD_ARG, "norm is NULL");
    if (actor->hidden != 32 && actor->hidden != 64) return bad(FG_ERR_BAD_ARG, "hidden must be 32 or 64 with LayerNorms");
    if (norm->in_norm && !actor_eps_ok(norm->in_eps)) return bad(FG_ERR_BAD_ARG, "in_eps must be positive and finite");
    if (!actor_eps_ok(norm->h1_eps)) return bad(FG_ERR_BAD_ARG, "h1_eps must be positive and finite");
    if (!actor_eps_ok(norm->h2_eps)) return bad(FG_ERR_BAD_ARG, "h2_eps must be positive and finite");
    const struct { const float* p; const char* name; } ptrs[] = {
        {norm->in_gamma, "in_gamma"}, {norm->in_beta, "in_beta"}, {norm->h1_gamma, "h1_gamma"},
        {norm->h1_beta, "h1_beta"},   {norm->h2_gamma, "h2_gamma"}, {norm->h2_beta, "h2_beta"}};
    for (const auto& q : ptrs)
        if ((uintptr_t)q.p & 3u) return bad(FG_ERR_BAD_ARG, "%s must be 4-byte aligned", q.name);
    return FG_OK;
}
// FgActorGru's and the hidden state's checks (no device touched): the layer and its four parameter tensors present, the state
// present where there are envs, norm_eps positive and finite (FG_ERR_BAD_ARG, the message naming the field); then the
// parameters 4-byte and the state 16-byte aligned (FG_ERR_ALIGNMENT)
static int actor_gru_check(const char* who, const FgActorGru* gru, const float* rnn_state, int B) {
    const ActorComplaint bad{who};
    if (!gru) return bad(FG_ERR_BAD_ARG, "gru is NULL");
    const struct { const float* p; const char* name; bool required; } ptrs[] = {
        {gru->w_ih, "w_ih", true}, {gru->w_hh, "w_hh", true}, {gru->b_ih, "b_ih", true},
        {gru->b_hh, "b_hh", true}, {gru->norm_gamma, "norm_gamma", false}, {gru->norm_beta, "norm_beta", false}};
    for (const auto& q : ptrs)
        if (q.required && !q.p) return bad(FG_ERR_BAD_ARG, "%s is NULL", q.name);
    if (!rnn_state && B > 0) return bad(FG_ERR_BAD_ARG, "rnn_state is NULL");
    if (!actor_eps_ok(gru->norm_eps)) return bad(FG_ERR_BAD_ARG, "norm_eps must be positive and finite");
    for (const auto& q : ptrs)
        if ((uintptr_t)q.p & 3u) return bad(FG_ERR_ALIGNMENT, "%s must be 4-byte aligned", q.name);
    if ((uintptr_t)rnn_state & 15u) return bad(FG_ERR_ALIGNMENT, "rnn_state must be 16-byte aligned");
    return FG_OK;
}
// FgActorInBn's checks (no device touched), in the name of the entry `who`; `member` >= 0: the per-agent entry's member, whose
// index the messages name.  FG_ERR_BAD_ARG for hidden = 128, a NULL mean or var, an eps that is not positive and finite;
// FG_ERR_ALIGNMENT for a mean, var, gamma or beta that is not 4-byte aligned.
static int actor_in_bn_check(const char* who, const FgActor& actor, const FgActorInBn& bn, int member) {
    const ActorComplaint bad{who, member};
    if (actor.hidden != 32 && actor.hidden != 64) return bad(FG_ERR_BAD_ARG, "hidden must be 32 or 64 with an input BatchNorm");
    if (!bn.mean) return bad(FG_ERR_BAD_ARG, "in_bn mean is NULL");
    if (!bn.var) return bad(FG_ERR_BAD_ARG, "in_bn var is NULL");
    if (!actor_eps_ok(bn.eps)) return bad(FG_ERR_BAD_ARG, "in_bn eps must be positive and finite");
    const struct { const float* p; const char* name; } ptrs[] = {
        {bn.mean, "mean"}, {bn.var, "var"}, {bn.gamma, "gamma"}, {bn.beta, "beta"}};
    for (const auto& q : ptrs)
        if ((uintptr_t)q.p & 3u) return bad(FG_ERR_ALIGNMENT, "in_bn %s must be 4-byte aligned", q.name);
    return FG_OK;
}
// FgActorOu's and the noise state's checks (no device touched), in the name of the entry `who`: FG_ERR_BAD_ARG naming the field
// for a NULL ou, a theta that is not finite or outside [0, 1], a mu, sigma or scale that is not finite, a negative sigma, a clip
// that is NaN or not positive (+inf: no clamp), a NULL state where there are envs; FG_ERR_ALIGNMENT for a state that is not
// 8-byte aligned.
static int actor_ou_check(const char* who, const FgActorOu* ou, const float* state, int B) {
    const ActorComplaint bad{who};
    if (!ou) return bad(FG_ERR_BAD_ARG, "ou is NULL");
    if (!(ou->theta >= 0.0f && ou->theta <= 1.0f)) return bad(FG_ERR_BAD_ARG, "theta must be in [0, 1]");
    if (!std::isfinite(ou->mu)) return bad(FG_ERR_BAD_ARG, "mu must be finite");
    if (!(ou->sigma >= 0.0f) || !std::isfinite(ou->sigma)) return bad(FG_ERR_BAD_ARG, "sigma must be finite and not negative");
    if (!std::isfinite(ou->scale)) return bad(FG_ERR_BAD_ARG, "scale must be finite");
    if (!(ou->clip > 0.0f)) return bad(FG_ERR_BAD_ARG, "clip must be positive (+inf: no clamp)");
    if (!state && B > 0) return bad(FG_ERR_BAD_ARG, "noise_state is NULL");
    if ((uintptr_t)state & 7u) return bad(FG_ERR_ALIGNMENT, "noise_state must be 8-byte aligned");
    return FG_OK;
}
// The categorical head's checks (no device touched), in the name of the entry `who`: FG_ERR_BAD_ARG for an actor with a tanh
// after its head, an action mode other than FG_ACT_ONEHOT5 / FG_ACT_INDEX, a NULL idx_seq where there are envs; FG_ERR_ALIGNMENT
// for an idx_seq or logp_seq that is not 4-byte aligned.
static int actor_cat_check(const char* who, const FgActor* actor, const HdActorHead& h, int B) {
    const ActorComplaint bad{who};
    if (actor->out_tanh != 0) return bad(FG_ERR_BAD_ARG, "out_tanh must be 0: the head's outputs are logits");
    if (h.mode != FG_ACT_ONEHOT5 && h.mode != FG_ACT_INDEX) return bad(FG_ERR_BAD_ARG, "act_mode must be FG_ACT_ONEHOT5 or FG_ACT_INDEX");
    if (!h.idx && B > 0) return bad(FG_ERR_BAD_ARG, "idx_seq is NULL");
    if (((uintptr_t)h.idx | (uintptr_t)h.logp) & 3u) return bad(FG_ERR_ALIGNMENT, "idx_seq and logp_seq must be 4-byte aligned");
    return FG_OK;
}
// The Gumbel head's checks (no device touched), in the name of the entry `who`; `actors` are the call's `n` members (1: the shared
// actor), each with a head of logits: FG_ERR_BAD_ARG for a tanh after a head, an action mode other than FG_ACT_ONEHOT5 /
// FG_ACT_INDEX, a NULL idx_seq where there are envs; FG_ERR_ALIGNMENT for an idx_seq that is not 4-byte aligned.
static int actor_gumbel_check(const char* who, const FgActor* actors, int n, const HdActorGumbel& h, int B) {
    const ActorComplaint bad{who};
    for (int i = 0; i < n; ++i)
        if (actors[i].out_tanh != 0) return bad(FG_ERR_BAD_ARG, "out_tanh must be 0: the head's outputs are logits");
    if (h.mode != FG_ACT_ONEHOT5 && h.mode != FG_ACT_INDEX) return bad(FG_ERR_BAD_ARG, "act_mode must be FG_ACT_ONEHOT5 or FG_ACT_INDEX");
    if (!h.idx && B > 0) return bad(FG_ERR_BAD_ARG, "idx_seq is NULL");
    if ((uintptr_t)h.idx & 3u) return bad(FG_ERR_ALIGNMENT, "idx_seq must be 4-byte aligned");
    return FG_OK;
}
// The checks of an hd-actor call before its buffers (no device touched): FG_OK, or the status of the first one that fails, in
// this order, which is ABI - params, (a 16-bit member: obs_format, the env pitch, log_std, N in {3, 9, 27}, hidden = 128,) B and K, N, the actor (per-agent: every member, then that it has member 0's hidden width
// and tanh flag), the norms, the recurrent layer with its state, the input BatchNorm(s), the OU noise with its state, the
// categorical head with its outputs, the Gumbel head with its output, log_std, logp.  The shared actor's
// checks name fg_rollout_hd_actor through the sample and norm entries too, the log_std checks fg_rollout_hd_actor_sample.
// Without log_std (the deterministic actor) `logp` is set to NULL.
static int hd_actor_check(const FgParams* params, HdActorCall& c, int B, int N, int K) {
    const char* const who = hd_actor_who(c);
    const char* const shared = hd_actor_entry[hd_actor_members(c) ? HD_ACTOR_PER_AGENT : HD_ACTOR_SHARED];
    int rc = check_params(params);
    if (rc) return rc;
    if (c.obs_format) {                                // the 16-bit members: what the writer and their instantiations ask for
        if (c.obs_format < 0) return fail(FG_ERR_BAD_ARG, "%s: obs_format must be FG_OBS_F16 or FG_OBS_BF16", who);
        if (params->obs_env_pitch != 0) return fail(FG_ERR_BAD_ARG, "%s: a padded env pitch (obs_env_pitch) is not supported", who);
        if (!c.cat.on && !c.log_std) return fail(FG_ERR_BAD_ARG, "%s: log_std is NULL", who);
        if (N != 3 && N != 9 && N != 27) return fail(FG_ERR_UNSUPPORTED_N, "%s: N must be 3, 9 or 27", who);
        if (c.actor && c.actor->hidden == 128) return fail(FG_ERR_BAD_ARG, "%s: hidden must be 32 or 64", who);
    }
    if (B < 0 || K < 1) return fail(FG_ERR_BAD_ARG, "%s: B >= 0 and K >= 1 required", shared);
    if (!actor_n_supported(N)) return fail(FG_ERR_UNSUPPORTED_N, "%s: N must be 3, 4, 8, 9, 16, 25, 27 or 32", shared);
    if (hd_actor_members(c)) {
        if (!c.actor) return fail(FG_ERR_BAD_ARG, "fg_rollout_hd_actor_per_agent: actors is NULL%s");
        char idx[16];
        for (int i = 0; i < N; ++i) {
            if ((rc = hd_actor_struct_check(params, &c.actor[i])) != FG_OK) return rc;
            if (c.actor[i].hidden != c.actor[0].hidden || (c.actor[i].out_tanh != 0) != (c.actor[0].out_tanh != 0)) {
                snprintf(idx, sizeof(idx), "%d", i);
                return fail(FG_ERR_BAD_ARG, "fg_rollout_hd_actor_per_agent: member %s differs from member 0 in hidden or out_tanh",
                            idx);
            }
        }
    } else if ((rc = hd_actor_struct_check(params, c.actor)) != FG_OK) {
        return rc;
    }
    if ((c.kind == HD_ACTOR_NORM || c.kind == HD_ACTOR_GRU) && (rc = actor_norm_check(who, c.actor, c.norm)) != FG_OK) return rc;
    if (c.kind == HD_ACTOR_GRU && (rc = actor_gru_check(who, c.gru, c.rnn_state, B)) != FG_OK) return rc;
    if (c.kind == HD_ACTOR_BN || c.kind == HD_ACTOR_BN_PER_AGENT) {
        if (!c.in_bn) return fail(FG_ERR_BAD_ARG, "%s: in_bn is NULL", who);
        if (c.kind == HD_ACTOR_BN) {
            if ((rc = actor_in_bn_check(who, *c.actor, *c.in_bn, -1)) != FG_OK) return rc;
        } else {
            for (int i = 0; i < N; ++i)
                if ((rc = actor_in_bn_check(who, c.actor[i], c.in_bn[i], i)) != FG_OK) return rc;
        }
    }
    if (c.noise.on && (rc = actor_ou_check(who, c.noise.ou, c.noise.state, B)) != FG_OK) return rc;
    if (c.cat.on && (rc = actor_cat_check(who, c.actor, c.cat, B)) != FG_OK) return rc;
    if (c.gumbel.on && (rc = actor_gumbel_check(who, c.actor, hd_actor_members(c) ? N : 1, c.gumbel, B)) != FG_OK) return rc;
    if (!c.log_std) {
        if (c.kind == HD_ACTOR_SAMPLE) return fail(FG_ERR_BAD_ARG, "fg_rollout_hd_actor_sample: log_std is NULL%s");
        c.logp = nullptr;
        return FG_OK;
    }
    if ((uintptr_t)c.log_std & 3u) return fail(FG_ERR_ALIGNMENT, "fg_rollout_hd_actor_sample: log_std must be 4-byte aligned%s");
    if ((uintptr_t)c.logp & 3u) return fail(FG_ERR_ALIGNMENT, "%s: logp_seq must be 4-byte aligned", who);
    return FG_OK;
}

// The kernels' operands from the caller's descriptions (checked: hd_actor_check).  The per-agent tables are zero past member N.
static ActorW actor_w(const FgActor& actor) {
    return {actor.w1, actor.b1, actor.w2, actor.b2, actor.w3, actor.b3, actor.out_tanh ? 1 : 0};
}
static ActorTab actor_tab(const FgActor* actors, int N) {
    ActorTab tab;
    memset(&tab, 0, sizeof(tab));
    for (int i = 0; i < N; ++i) {
        tab.w1[i] = actors[i].w1; tab.b1[i] = actors[i].b1; tab.w2[i] = actors[i].w2;
        tab.b2[i] = actors[i].b2; tab.w3[i] = actors[i].w3; tab.b3[i] = actors[i].b3;
    }
    tab.out_tanh = actors[0].out_tanh ? 1 : 0;
    return tab;
}
static ActorBnW actor_bn_w(const FgActorInBn& bn) { return {bn.mean, bn.var, bn.gamma, bn.beta, bn.eps}; }
static ActorBnTab actor_bn_tab(const FgActorInBn* bns, int N) {
    ActorBnTab btab;
    memset(&btab, 0, sizeof(btab));
    for (int i = 0; i < N; ++i) {
        btab.mean[i] = bns[i].mean; btab.var[i] = bns[i].var; btab.gamma[i] = bns[i].gamma;
        btab.beta[i] = bns[i].beta; btab.eps[i] = bns[i].eps;
    }
    return btab;
}
static ActorOuW actor_ou_w(const HdActorNoise& n) {
    return {n.ou->theta, n.ou->mu, n.ou->sigma, n.ou->scale, n.ou->clip, n.state};
}
static ActorNormW actor_norm_w(const FgActorNorm& norm) {
    const bool in_norm = norm.in_norm != 0;
    return {in_norm ? norm.in_gamma : nullptr, in_norm ? norm.in_beta : nullptr, norm.h1_gamma, norm.h1_beta,
            norm.h2_gamma, norm.h2_beta, in_norm ? norm.in_eps : 1.0f, norm.h1_eps, norm.h2_eps, in_norm ? 1 : 0};
}
static ActorGruW actor_gru_w(const HdActorCall& c) {
    const FgActorGru& g = *c.gru;
    return {g.w_ih, g.w_hh, g.b_ih, g.b_hh, g.norm_gamma, g.norm_beta, g.norm_eps, c.rnn_state,
            c.states_entry ? c.rnn_states : nullptr, c.states_entry ? c.states_every : 1};
}

// The one N x H grid of the formation_hd_env actor kernels: launch(n, h) with N and H as the `value` of the arguments' types,
// or UNSUPPORTED_N in `who`'s name when N is not in the list.  MAXH is the widest H of the caller's kernels: `hidden` is 32,
// 64 or - MAXH == 128 only - 128 (actor_struct_check, actor_norm_check), and no launch(n, 128) is instantiated below that.
template <int MAXH, class F>
static int actor_nh_dispatch(int N, int hidden, const char* who, F&& launch) {
#define FG_ACTOR(NN)                                                                      \
    if (N == NN) {                                                                        \
        if (hidden == 32) return launch(IntC<NN>{}, IntC<32>{});                          \
        if constexpr (MAXH == 128) if (hidden != 64) return launch(IntC<NN>{}, IntC<128>{}); \
        return launch(IntC<NN>{}, IntC<64>{});                                            \
    }
    FG_ACTOR(3) FG_ACTOR(4) FG_ACTOR(8) FG_ACTOR(9) FG_ACTOR(16) FG_ACTOR(25) FG_ACTOR(27) FG_ACTOR(32)
#undef FG_ACTOR
    return fail(FG_ERR_UNSUPPORTED_N, "%s: N must be 3, 4, 8, 9, 16, 25, 27 or 32", who);
}
// the call's member of the family F at <NC, H>: `w` are the family's operands, and each case adds its member's arguments
template <int NC, int H, class F, class... W>
static int launch_hd_actor(const Args& a, const HdActorCall& c, hipStream_t st, const W&... w) {
    const ActorOuW ow = c.noise.on ? actor_ou_w(c.noise) : ActorOuW{};
    const ActorCatW cw = {c.cat.mode, c.cat.greedy ? 1 : 0, c.cat.idx, c.cat.logp};
    const ActorGumW gum = {c.gumbel.mode, c.gumbel.explore ? 1 : 0, c.gumbel.idx};
    const int fmt = c.obs_format == FG_OBS_F16 ? FG_WR_OBS_F16 : FG_WR_OBS_BF16;      // (the writer's, read by the 16-bit members)
    switch (hd_actor_member(c)) {
    case ACTOR_GAUSS: return launch_hd_member<ACTOR_GAUSS, NC, H, F>(a, st, w..., c.log_std, c.logp);
    case ACTOR_OU: return launch_hd_member<ACTOR_OU, NC, H, F>(a, st, w..., ow);
    case ACTOR_CAT: return launch_hd_member<ACTOR_CAT, NC, H, F>(a, st, w..., cw);
    case ACTOR_GAUSS16: return launch_hd_member<ACTOR_GAUSS16, NC, H, F>(a, st, w..., c.log_std, c.logp, fmt);
    case ACTOR_CAT16: return launch_hd_member<ACTOR_CAT16, NC, H, F>(a, st, w..., cw, fmt);
    case ACTOR_GUMBEL: return launch_hd_member<ACTOR_GUMBEL, NC, H, F>(a, st, w..., gum);
    default: return launch_hd_member<ACTOR_DET, NC, H, F>(a, st, w...);
    }
}
// the family KIND's kernel for the call's (N, hidden), with the family's operands `w`
template <HdActorKind KIND, class... W>
static int hd_actor_run(const Args& a, const HdActorCall& c, hipStream_t st, const W&... w) {
    const char* const who = c.kind == HD_ACTOR_SAMPLE ? hd_actor_entry[HD_ACTOR_SHARED] : hd_actor_who(c);
    return actor_nh_dispatch<HdActorFamily<KIND>::max_h>(a.N, c.actor[0].hidden, who, [&](auto n, auto h) {
        return launch_hd_actor<decltype(n)::value, decltype(h)::value, HdActorFamily<KIND>>(a, c, st, w...);
    });
}
// a checked call (hd_actor_check) to its kernel; a describe twin passes a NULL stream
static int hd_actor_dispatch(const Args& a, const HdActorCall& c, hipStream_t st) {
    switch (c.kind) {
    case HD_ACTOR_PER_AGENT: return hd_actor_run<HD_ACTOR_PER_AGENT>(a, c, st, actor_tab(c.actor, a.N));
    case HD_ACTOR_NORM: return hd_actor_run<HD_ACTOR_NORM>(a, c, st, actor_w(*c.actor), actor_norm_w(*c.norm));
    case HD_ACTOR_GRU: return hd_actor_run<HD_ACTOR_GRU>(a, c, st, actor_w(*c.actor), actor_norm_w(*c.norm), actor_gru_w(c));
    case HD_ACTOR_BN: return hd_actor_run<HD_ACTOR_BN>(a, c, st, actor_w(*c.actor), actor_bn_w(*c.in_bn));
    case HD_ACTOR_BN_PER_AGENT:
        return hd_actor_run<HD_ACTOR_BN_PER_AGENT>(a, c, st, actor_tab(c.actor, a.N), actor_bn_tab(c.in_bn, a.N));
    default: return hd_actor_run<HD_ACTOR_SHARED>(a, c, st, actor_w(*c.actor));        // HD_ACTOR_SHARED, HD_ACTOR_SAMPLE
    }
}

// An fg_rollout_hd_actor* entry: the call's checks, the buffers', then the launch
static int rollout_actor_impl(const FgParams* params, HdActorCall c, int B, int N, int K, const HdRollout& r, int obs_every,
                              void* stream) {
    int rc = hd_actor_check(params, c, B, N, K);
    if (rc || (rc = rollout_buffers_check("fg_rollout_hd_actor", r))) return rc;
    if (c.states_entry) {                              // the record's own checks, after every one the entry inherits
        const char* const who = hd_actor_who(c);
        if (c.states_every < 1) return fail(FG_ERR_BAD_ARG, "%s: states_every >= 1 required", who);
        if (!c.rnn_states && B > 0) return fail(FG_ERR_BAD_ARG, "%s: rnn_states is NULL", who);
        if ((uintptr_t)c.rnn_states & 15u) return fail(FG_ERR_ALIGNMENT, "%s: rnn_states must be 16-byte aligned", who);
    }
    if (B == 0) return FG_OK;
    const DeviceGuard device_guard(stream, r.pos_x);
    Args a;
    if ((rc = hd_args(&a, params, B, N, K, obs_every, 1, 1))) return rc;
    hd_buffers(&a, r);
    a.act_out = r.act_seq;
    return hd_actor_dispatch(a, c, (hipStream_t)stream);
}

// the describe twin `who` of the call `c`: the out buffer's check, the call's own checks, then the dry run of its dispatch
static int describe_actor_impl(const char* who, const FgParams* params, HdActorCall c, int B, int N, int K, int obs_every,
                               char* out, int out_len) {
    if (!out || out_len < 2) return fail(FG_ERR_BAD_ARG, "%s: out buffer required", who);
    out[0] = 0;
    int rc = hd_actor_check(params, c, B, N, K);
    if (rc) return rc;
    if (B <= 0) return fail(FG_ERR_BAD_ARG, "fg_describe_actor_launch: B > 0 required%s");
    Args a;
    if ((rc = hd_args(&a, params, B, N, K, obs_every, 1, 1))) return rc;
    const DescribeScope describing(out, out_len);
    return hd_actor_dispatch(a, c, nullptr);
}

// ---- closed loop with the caller's MLP actor in the landmark scenarios (fg_scn_lane_actor_kernel.hpp) ----
// log_std == NULL: scn_lane_actor (the deterministic actor); else scn_lane_actor_gauss (the Gaussian actor)
template <int KIND, int NN, int LL, int MM, int NBR, int H>
static int launch_scn_actor(const ScnArgs& a, const ActorW& w, float* act_out, const float* log_std, float* logp, hipStream_t st) {
    static_assert(scn_actor_lds_bytes(KIND, NN, LL, MM, NBR, H, true) <= 160 * 1024, "scenario actor rollout LDS");
    char targs[48];
    snprintf(targs, sizeof(targs), "%d,%d,%d,%d,%d,%d", KIND, NN, LL, MM, NBR, H);
    return launch_actor_pair<&scn_lane_actor<KIND, NN, LL, MM, NBR, H>, &scn_lane_actor_gauss<KIND, NN, LL, MM, NBR, H>>(
        "scn_lane_actor", "scn_lane_actor_gauss", targs, "threads", 8 * (((a.B + FG_SCN_ACTOR_ENVS - 1) / FG_SCN_ACTOR_ENVS + 7) / 8),
        FG_SCN_ACTOR_THREADS, FG_SCN_ACTOR_ENVS, scn_actor_lds_bytes(KIND, NN, LL, MM, NBR, H, log_std != nullptr),
        "scenario actor rollout launch failed: %s", st, log_std, logp, a, w, act_out);
}

// the checks both scenario-actor entries share (no device touched): FG_OK, or the status of the first one that fails
static int scn_actor_check(const FgParams* params, const FgScenario* sc, const FgActor* actor, const float* log_std,
                           const float* logp, int B, int N, int K) {
    int rc = check_params(params);
    if (rc) return rc;
    if (!sc) return fail(FG_ERR_BAD_ARG, "fg_rollout_scenario_actor: scenario descriptor is NULL%s");
    if (B < 0 || K < 1) return fail(FG_ERR_BAD_ARG, "fg_rollout_scenario_actor: B >= 0 and K >= 1 required%s");
    if (sc->kind < FG_SCN_BASIC || sc->kind > FG_SCN_OBSTACLE)
        return fail(FG_ERR_BAD_ARG, "fg_rollout_scenario_actor: unknown scenario kind%s");
    if ((rc = actor_struct_check(actor, "fg_rollout_scenario_actor", 64, "32 or 64", (uintptr_t)log_std | (uintptr_t)logp,
                                 "weights, log_std and logp")) != FG_OK)
        return rc;
    if (!log_std && logp) return fail(FG_ERR_BAD_ARG, "fg_rollout_scenario_actor: logp without log_std%s");
    if (params->agent_props || params->comm_state || sc->variant == 1)
        return fail(FG_ERR_BAD_ARG, "fg_rollout_scenario_actor: per-agent properties, communication and variant 1 are not supported%s");
    return FG_OK;
}

static int scn_actor_dispatch(const ScnArgs& a, const FgActor& actor, float* act_out, const float* log_std, float* logp,
                              hipStream_t st) {
    const ActorW w = actor_w(actor);
    const int L = a.sc.num_landmarks, M = a.sc.num_obstacles;
    const int nbr = a.sc.kind == FG_SCN_PARTIAL ? a.sc.num_obs : a.N - 1;
#define FG_SCN_ACTOR(KIND, NN, LL, MM, NBR, WIDE)                                                            \
    if (a.sc.kind == KIND && a.N == NN && L == LL && M == MM && nbr == NBR)                                  \
        return actor.hidden == 32 ? launch_scn_actor<KIND, NN, LL, MM, NBR, 32>(a, w, act_out, log_std, logp, st) \
                                  : launch_scn_actor<KIND, NN, LL, MM, NBR, 64>(a, w, act_out, log_std, logp, st);
    FG_SCN_SHAPES(FG_SCN_ACTOR)
#undef FG_SCN_ACTOR
    return fail(FG_ERR_UNSUPPORTED_N, "fg_rollout_scenario_actor: (scenario, N, landmarks, obstacles, num_obs) is not one of the reference shapes%s");
}

// ---- discounted returns of C candidate action sequences from the current state (fg_returns_kernel.hpp) ----
// the checks fg_rollout_hd_returns (`who`; fg_rollout_hd_returns_sampled likewise) and its dry run share (no pointer, no
// device): FG_OK, or the status of the first that fails
static int returns_check(const FgParams* params, int B, int N, int K, int C, float gamma, const char* who = "fg_rollout_hd_returns") {
    const int rc = check_params(params);
    if (rc) return rc;
    if (B < 0 || K < 1 || C < 1) return fail(FG_ERR_BAD_ARG, "%s: B >= 0, K >= 1 and C >= 1 required", who);
    if (!(gamma >= 0.0f && gamma <= 1.0f)) return fail(FG_ERR_BAD_ARG, "%s: gamma must be a finite number in [0, 1]", who);
    if (world_options_set(*params))
        return fail(FG_ERR_BAD_ARG, "%s: World options, per-agent properties and communication are not supported", who);
    if (!actor_n_supported(N)) return fail(FG_ERR_UNSUPPORTED_N, "%s: N must be 3, 4, 8, 9, 16, 25, 27 or 32", who);
    if ((long long)B * C > 0x7fffffffLL) return fail(FG_ERR_BAD_ARG, "%s: B * C must be below 2^31", who);
    return FG_OK;
}
// ... and those on the buffers of the two entries, `src` being the one the actions come from (act / mean); fills `a`
static int returns_args(const char* who, const char* aligned_fmt, ReturnsArgs* a, const FgParams* params, int B, int K, int C,
                        float gamma, const float* pos_x, const float* pos_y, const float* vel_x, const float* vel_y,
                        const float* ideal_shape, const float* ideal_vel, const int32_t* step, const float* src, float* ret,
                        float* indiv_ret, int32_t* steps) {
    if (!pos_x || !pos_y || !vel_x || !vel_y || !ideal_shape || !ideal_vel || !step || !src || !ret) return null_pointer(who);
    if ((((uintptr_t)src | (uintptr_t)ideal_shape | (uintptr_t)ideal_vel) & 7u) ||
        (((uintptr_t)pos_x | (uintptr_t)pos_y | (uintptr_t)vel_x | (uintptr_t)vel_y | (uintptr_t)step | (uintptr_t)ret |
          (uintptr_t)indiv_ret | (uintptr_t)steps) & 3u))
        return fail(FG_ERR_ALIGNMENT, aligned_fmt, who);
    memset(a, 0, sizeof(*a));
    a->p = *params; a->B = B; a->K = K; a->C = C; a->gamma = gamma;
    a->px = pos_x; a->py = pos_y; a->vx = vel_x; a->vy = vel_y; a->shape = ideal_shape; a->ivel = ideal_vel; a->step = step;
    a->ret = ret; a->indiv_ret = indiv_ret; a->steps = steps;
    return FG_OK;
}
// One geometry per agent count (fg_returns_kernel.hpp): the lane group of step_kernel and the rollout producers, 256 threads.
// `A` is ReturnsArgs (returns_kernel: the actions read) or ReturnsSampledArgs (returns_sampled_kernel: the actions drawn,
// fg_planner_kernels.hpp) - the same geometry for both.
static const ReturnsArgs& returns_of(const ReturnsArgs& a) { return a; }
static const ReturnsArgs& returns_of(const ReturnsSampledArgs& a) { return a.r; }
static const ReturnsArgs& returns_of(const ReturnsSampledStdArgs& a) { return a.r; }
template <int NC, int G, class A>
static int launch_returns_v(const A& a, hipStream_t st) {
    constexpr int T = 256, PW = T / G;
    constexpr int lds = returns_lds_bytes<NC, G, T>();
    constexpr bool sampled = std::is_same<A, ReturnsSampledArgs>::value;
    constexpr bool sampled_std = std::is_same<A, ReturnsSampledStdArgs>::value;     // (a sigma per element)
    const unsigned grid = (unsigned)(((long long)returns_of(a).B * returns_of(a).C + PW - 1) / PW);
    if (describe("%s<%d,%d,%d> grid %u block %d lds %d; ",
                 sampled_std ? "returns_sampled_std_kernel" : sampled ? "returns_sampled_kernel" : "returns_kernel", NC, G, T, grid, T, lds))
        return FG_OK;
    if constexpr (sampled_std)
        return launch<&returns_sampled_std_kernel<NC, G, T>>(grid, T, lds, st, "sampled returns launch failed: %s", a);
    else if constexpr (sampled) return launch<&returns_sampled_kernel<NC, G, T>>(grid, T, lds, st, "sampled returns launch failed: %s", a);
    else return launch<&returns_kernel<NC, G, T>>(grid, T, lds, st, "returns launch failed: %s", a);
}
template <class A>
static int returns_dispatch(const A& a, int N, hipStream_t st) {
#define FG_RETURNS(NN, G) if (N == NN) return launch_returns_v<NN, G>(a, st);
    FG_RETURNS(3, 4) FG_RETURNS(4, 4) FG_RETURNS(8, 8) FG_RETURNS(9, 16) FG_RETURNS(16, 16)
    FG_RETURNS(25, 32) FG_RETURNS(27, 32) FG_RETURNS(32, 32)
#undef FG_RETURNS
    return fail(FG_ERR_UNSUPPORTED_N, "returns launch: N must be 3, 4, 8, 9, 16, 25, 27 or 32%s");   // (unreachable after returns_check)
}

// ---- a sampling planner's candidates (fg_planner_kernels.hpp) ----
// the scalars every planner entry shares, after its own check of params: FG_OK, or the status of the first that fails
static int plan_check(const char* who, int B, int N, int K, int C, float sigma) {
    if (B < 0 || K < 1 || C < 1) return fail(FG_ERR_BAD_ARG, "%s: B >= 0, K >= 1 and C >= 1 required", who);
    if (N < 1 || N > FG_PLAN_MAX_N) return fail(FG_ERR_BAD_ARG, "%s: 1 <= N <= 2^12 required", who);
    if (C > FG_PLAN_MAX_C) return fail(FG_ERR_BAD_ARG, "%s: C <= 2^17 required", who);
    if (!(sigma >= 0.0f) || !std::isfinite(sigma)) return fail(FG_ERR_BAD_ARG, "%s: sigma must be a finite number >= 0", who);
    return FG_OK;
}
static PlanDraw plan_draw_of(const FgParams* params, uint64_t noise_offset, float sigma, float clip) {
    PlanDraw d;
    d.seed = params->seed; d.noise_offset = noise_offset; d.env_index_base = (uint32_t)params->env_index_base;
    d.sigma = sigma; d.clip = clip;
    return d;
}
// one thread per element of an element-wise planner launch: the grid, or 0 when `count` threads are more than a launch holds
static unsigned plan_grid(long long count) {
    const long long grid = (count + 255) / 256;
    return grid > 0x7fffffffLL ? 0u : (unsigned)grid;
}
// the dry run of a sampled scoring entry (`who`; `A` its kernel's arguments): that entry's checks before the buffers, then
// its dispatch.  Touches no device.
template <class A>
static int describe_sampled(const char* name, const char* who, const FgParams* params, int B, int N, int K, int C, char* text,
                            int cap) {
    if (!text || cap < 2) return fail(FG_ERR_BAD_ARG, "%s: out buffer required", name);
    text[0] = 0;
    int rc = returns_check(params, B, N, K, C, 1.0f, who);
    if (rc || (rc = plan_check(who, B, N, K, C, 0.0f)) || B == 0) return rc;
    A a;
    memset(&a, 0, sizeof(a));
    a.r.p = *params; a.r.B = B; a.r.K = K; a.r.C = C; a.r.gamma = 1.0f;
    const DescribeScope describing(text, cap);
    return returns_dispatch(a, N, nullptr);
}

extern "C" {

int fg_abi_version(void) { return FG_ABI_VERSION; }

// ---- placed device memory: separately created physical chunks, mapped into fresh address ranges (HIP virtual memory
// management).  Discipline: (1) a chunk is mapped at ONE address at a time (no aliases); (2) the device is drained before
// any mapping goes away; (3) an address range that has held a mapping is NEVER used again in this process: on this stack
// (ROCm 7.2, MI355X) hipMemUnmap leaves the GPU's translations of the range behind, and a later mapping at the same
// address has most of its accesses land in the chunks that were mapped there before (profiles/r03_place/va_reuse_check.txt:
// 73-100 % of the old chunks overwritten).  So reservations are not handed back (hipMemAddressFree would let the very
// next reservation land on them); they cost address space only - the physical chunks are released as soon as they are
// not needed.
namespace {
struct Arena {
    int dev = 0;
    size_t chunk = 0, n = 0;
    std::vector<hipMemGenericAllocationHandle_t> handle;
    std::vector<char> live;                             // handle exists
    std::vector<int> mapped_in;                         // index of the mapping that holds the chunk, -1 = unmapped
    struct Mapping { char* base; std::vector<uint32_t> chunks; };
    std::vector<Mapping> maps;                          // slots; base == nullptr: free slot
};
}  // namespace

// Before any chunk is unmapped or released the whole device is drained: work on ANY stream may still be using the
// addresses that are about to go away.
static void drain_device(int dev) {
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
    (void)hipDeviceSynchronize();
    if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
}

static std::atomic<unsigned long long> g_retired_address_bytes{0};   // reservations retired for good (discipline 3)

static void arena_unmap_slot(Arena* a, size_t slot) {
    Arena::Mapping& m = a->maps[slot];
    if (!m.base) return;
    for (size_t j = 0; j < m.chunks.size(); ++j) {
        (void)hipMemUnmap(m.base + j * a->chunk, a->chunk);
        a->mapped_in[m.chunks[j]] = -1;
    }
    g_retired_address_bytes.fetch_add((unsigned long long)(m.chunks.size() * a->chunk));   // the reservation stays: never reused
    m.base = nullptr; m.chunks.clear();
}

// An address range that has held a mapping is retired, not freed (discipline 3): a process-wide budget keeps a long-lived
// caller that places buffers again and again from running the 128 TiB address space dry (then arenas are refused and the
// caller falls back to ordinary allocations, which is what placement.py does on any arena failure).
static const unsigned long long kRetiredAddressBudget = 64ull << 40;

int fg_arena_create(int device, uint64_t bytes, uint64_t chunk_bytes, void** arena, uint64_t* chunk_out, uint32_t* chunks_out) {
    if (!arena || bytes == 0) return fail(FG_ERR_BAD_ARG, "fg_arena_create: arena and bytes > 0 required%s");
    if (g_retired_address_bytes.load() > kRetiredAddressBudget)
        return fail(FG_ERR_HIP, "fg_arena_create: the address-space budget of retired reservations (64 TiB) is spent%s");
    hipMemAllocationProp prop;
    memset(&prop, 0, sizeof(prop));
    prop.type = hipMemAllocationTypePinned;
    prop.location.type = hipMemLocationTypeDevice;
    prop.location.id = device;
    size_t gran = 0;
    hipError_t err = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended);
    if (err != hipSuccess || gran == 0) return fail(FG_ERR_HIP, "hipMemGetAllocationGranularity failed: %s", hipGetErrorString(err));
    size_t chunk = chunk_bytes ? (size_t)chunk_bytes : ((size_t)1 << 30);
    chunk = (chunk + gran - 1) / gran * gran;
    Arena* a = new Arena();
    a->dev = device; a->chunk = chunk; a->n = ((size_t)bytes + chunk - 1) / chunk;
    a->handle.resize(a->n); a->live.assign(a->n, 0); a->mapped_in.assign(a->n, -1);
    for (size_t i = 0; i < a->n; ++i) {
        err = hipMemCreate(&a->handle[i], chunk, &prop, 0);
        if (err != hipSuccess) break;
        a->live[i] = 1;
    }
    // Every chunk is mapped once, in index order, and unmapped again (the reservation is retired, see above): a chunk has
    // its physical place from here on, whatever selection it is mapped in later.  (Where that place is, the driver
    // decides: holding memory between two groups of chunks while they are created does NOT put them reliably apart -
    // profiles/r04_place/spread_rule*.txt - which is why selections are timed, not composed by rule.)
    void* va = nullptr;
    size_t mapped = 0;
    if (err == hipSuccess) err = hipMemAddressReserve(&va, a->n * chunk, 0, nullptr, 0);
    if (err == hipSuccess) {
        for (; mapped < a->n; ++mapped) {
            err = hipMemMap((char*)va + mapped * chunk, chunk, 0, a->handle[mapped], 0);
            if (err != hipSuccess) break;
        }
        if (err == hipSuccess) {
            hipMemAccessDesc desc;
            memset(&desc, 0, sizeof(desc));
            desc.location.type = hipMemLocationTypeDevice;
            desc.location.id = device;
            desc.flags = hipMemAccessFlagsProtReadWrite;
            err = hipMemSetAccess(va, a->n * chunk, &desc, 1);
        }
        drain_device(device);
        for (size_t i = 0; i < mapped; ++i) (void)hipMemUnmap((char*)va + i * chunk, chunk);
        g_retired_address_bytes.fetch_add((unsigned long long)(a->n * chunk));
    }
    if (err != hipSuccess) {
        const int rc = fail(FG_ERR_HIP, "fg_arena_create: %s", hipGetErrorString(err));
        (void)hipGetLastError();
        for (size_t i = 0; i < a->n; ++i) if (a->live[i]) (void)hipMemRelease(a->handle[i]);
        delete a;
        return rc;
    }
    *arena = a;
    if (chunk_out) *chunk_out = chunk;
    if (chunks_out) *chunks_out = (uint32_t)a->n;
    return FG_OK;
}

int fg_arena_map(void* arena, const uint32_t* chunk_index, uint32_t count, void** base) {
    Arena* a = (Arena*)arena;
    if (!a || !chunk_index || !base || count == 0) return fail(FG_ERR_BAD_ARG, "fg_arena_map: arena, indices and base required%s");
    std::vector<char> seen(a->n, 0);
    for (uint32_t j = 0; j < count; ++j) {
        const uint32_t c = chunk_index[j];
        if (c >= a->n || !a->live[c]) return fail(FG_ERR_BAD_ARG, "fg_arena_map: chunk index out of range or released%s");
        if (a->mapped_in[c] >= 0 || seen[c]) return fail(FG_ERR_BAD_ARG, "fg_arena_map: a chunk is mapped at one address at a time%s");
        seen[c] = 1;
    }
    if (g_retired_address_bytes.load() > kRetiredAddressBudget)
        return fail(FG_ERR_HIP, "fg_arena_map: the address-space budget of retired reservations (64 TiB) is spent%s");
    void* va = nullptr;
    hipError_t err = hipMemAddressReserve(&va, (size_t)count * a->chunk, 0, nullptr, 0);
    if (err != hipSuccess) return fail(FG_ERR_HIP, "hipMemAddressReserve failed: %s", hipGetErrorString(err));
    uint32_t done = 0;
    for (; done < count; ++done) {
        err = hipMemMap((char*)va + (size_t)done * a->chunk, a->chunk, 0, a->handle[chunk_index[done]], 0);
        if (err != hipSuccess) break;
    }
    if (err == hipSuccess) {
        hipMemAccessDesc desc;
        memset(&desc, 0, sizeof(desc));
        desc.location.type = hipMemLocationTypeDevice;
        desc.location.id = a->dev;
        desc.flags = hipMemAccessFlagsProtReadWrite;
        err = hipMemSetAccess(va, (size_t)count * a->chunk, &desc, 1);
    }
    if (err != hipSuccess) {
        const int rc = fail(FG_ERR_HIP, "fg_arena_map: %s", hipGetErrorString(err));
        (void)hipGetLastError();
        for (uint32_t j = 0; j < done; ++j) (void)hipMemUnmap((char*)va + (size_t)j * a->chunk, a->chunk);
        g_retired_address_bytes.fetch_add((unsigned long long)count * a->chunk);   // held a mapping: retired, not freed
        return rc;
    }
    size_t slot = a->maps.size();
    for (size_t k = 0; k < a->maps.size(); ++k) if (!a->maps[k].base) { slot = k; break; }
    if (slot == a->maps.size()) a->maps.push_back(Arena::Mapping{nullptr, {}});
    a->maps[slot].base = (char*)va;
    a->maps[slot].chunks.assign(chunk_index, chunk_index + count);
    for (uint32_t j = 0; j < count; ++j) a->mapped_in[chunk_index[j]] = (int)slot;
    drain_device(a->dev);                               // the page-table work is complete before the caller launches into it
    *base = va;
    return FG_OK;
}

int fg_arena_unmap(void* arena, void* base) {
    Arena* a = (Arena*)arena;
    if (!a || !base) return fail(FG_ERR_BAD_ARG, "fg_arena_unmap: arena and base required%s");
    for (size_t k = 0; k < a->maps.size(); ++k)
        if (a->maps[k].base == (char*)base) {
            drain_device(a->dev);
            arena_unmap_slot(a, k);
            return FG_OK;
        }
    return fail(FG_ERR_BAD_ARG, "fg_arena_unmap: not a mapping of this arena%s");
}

// Shrinks a mapping to the window [first, first + count) of its chunks: the chunks outside are unmapped (their part of the
// reservation is retired), the window stays where it is.  The probe keeps its winner this way when it lies in the mapping it
// timed last, instead of mapping it once more at a fresh address.
int fg_arena_keep_window(void* arena, void* base, uint32_t first, uint32_t count, void** new_base) {
    Arena* a = (Arena*)arena;
    if (!a || !base || !new_base || count == 0) return fail(FG_ERR_BAD_ARG, "fg_arena_keep_window: arena, base, new_base and count > 0 required%s");
    for (size_t k = 0; k < a->maps.size(); ++k) {
        Arena::Mapping& m = a->maps[k];
        if (m.base != (char*)base) continue;
        if ((size_t)first + count > m.chunks.size()) return fail(FG_ERR_BAD_ARG, "fg_arena_keep_window: window beyond the mapping%s");
        drain_device(a->dev);
        size_t gone = 0;
        for (size_t j = 0; j < m.chunks.size(); ++j) {
            if (j >= first && j < (size_t)first + count) continue;
            (void)hipMemUnmap(m.base + j * a->chunk, a->chunk);
            a->mapped_in[m.chunks[j]] = -1;
            ++gone;
        }
        g_retired_address_bytes.fetch_add((unsigned long long)(gone * a->chunk));
        std::vector<uint32_t> kept(m.chunks.begin() + first, m.chunks.begin() + first + count);
        m.base += (size_t)first * a->chunk;
        m.chunks.swap(kept);
        *new_base = m.base;
        return FG_OK;
    }
    return fail(FG_ERR_BAD_ARG, "fg_arena_keep_window: not a mapping of this arena%s");
}

uint64_t fg_arena_retired_address_bytes(void) { return (uint64_t)g_retired_address_bytes.load(); }

int fg_arena_trim(void* arena) {
    Arena* a = (Arena*)arena;
    if (!a) return fail(FG_ERR_BAD_ARG, "fg_arena_trim: arena is NULL%s");
    for (size_t i = 0; i < a->n; ++i)
        if (a->live[i] && a->mapped_in[i] < 0) { (void)hipMemRelease(a->handle[i]); a->live[i] = 0; }
    return FG_OK;
}

int fg_arena_destroy(void* arena) {
    Arena* a = (Arena*)arena;
    if (!a) return FG_OK;
    drain_device(a->dev);
    for (size_t k = 0; k < a->maps.size(); ++k) arena_unmap_slot(a, k);
    for (size_t i = 0; i < a->n; ++i) if (a->live[i]) (void)hipMemRelease(a->handle[i]);
    delete a;
    return FG_OK;
}

const char* fg_last_error(void) { return g_err; }

int fg_launch_device(void* stream, const void* data) { return resolve_device(stream, data); }

int fg_kernel_config(int N, int* threads, int* envs_per_wg, int* lds_bytes) {
    if (const int rc = generic_n_check(N)) return rc;
    Geometry g;
    geometry_for(N, &g);
    if (threads) *threads = g.T;
    if (envs_per_wg) *envs_per_wg = g.E;
    if (lds_bytes) *lds_bytes = g.lds;
    return FG_OK;
}

int64_t fg_step_hd_bytes(int N) { return 24LL * N * N + 53LL * N + 16LL; }

int fg_step_hd(const FgParams* params, int B, int N,
               float* pos_x, float* pos_y, float* vel_x, float* vel_y,
               const float* act, float* ideal_shape, float* ideal_vel, int32_t* step,
               float* obs, float* reward, float* indiv_reward, uint8_t* done,
               int32_t* near_lm, int32_t* near_ag, int32_t* hd_idx, void* stream) {
    const DeviceGuard device_guard(stream, pos_x);
    Args a;
    const int rc = step_hd_describe(params, B, N, pos_x, pos_y, vel_x, vel_y, act, ideal_shape, ideal_vel, step,
                                    obs, reward, indiv_reward, done, near_lm, near_ag, hd_idx, &a);
    if (rc) return rc;
    return step_hd_dispatch(a, (hipStream_t)stream);
}

int fg_step_hd_plan(const FgParams* params, int B, int N,
                    float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                    const float* act, float* ideal_shape, float* ideal_vel, int32_t* step,
                    float* obs, float* reward, float* indiv_reward, uint8_t* done,
                    int32_t* near_lm, int32_t* near_ag, int32_t* hd_idx, void* stream, void** plan) {
    if (!plan) return fail(FG_ERR_BAD_ARG, "fg_step_hd_plan: plan is NULL%s");
    Args a;
    const int rc = step_hd_describe(params, B, N, pos_x, pos_y, vel_x, vel_y, act, ideal_shape, ideal_vel, step,
                                    obs, reward, indiv_reward, done, near_lm, near_ag, hd_idx, &a);
    if (rc) return rc;
    StepPlan* sp = new StepPlan();
    sp->a = a; sp->stream = (hipStream_t)stream;
    sp->device = visible_devices() < 2 ? -1 : resolve_device(stream, pos_x);
    *plan = sp;
    return FG_OK;
}

int fg_plan_launch(void* plan, uint64_t rng_offset) {
    StepPlan* sp = (StepPlan*)plan;
    if (!sp) return fail(FG_ERR_BAD_ARG, "fg_plan_launch: plan is NULL%s");
    const DeviceGuard device_guard(sp->device);       // resolved at plan time: no query per step
    sp->a.p.rng_offset = rng_offset;
    return step_hd_dispatch(sp->a, sp->stream);
}

int fg_plan_destroy(void* plan) {
    delete (StepPlan*)plan;
    return FG_OK;
}

int fg_physics_step(const FgParams* params, int B, int N,
                    float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                    const float* act, void* stream) {
    const DeviceGuard device_guard(stream, pos_x);
    int rc = check_params(params);
    if (rc) return rc;
    if (B == 0) return FG_OK;                         // an empty batch is a no-op (e.g. a rank that owns no envs)
    if (B < 0) return fail(FG_ERR_BAD_ARG, "B must be >= 0%s");
    if ((rc = generic_n_check(N))) return rc;
    if (!pos_x || !pos_y || !vel_x || !vel_y || !act) return null_pointer("fg_physics_step");
    if ((uintptr_t)act & 7u) return fail(FG_ERR_ALIGNMENT, "act must be 8-byte aligned%s");
    Args a;
    if ((rc = hd_args(&a, params, B, N, 1, 1, 1, 0))) return rc;
    a.p.auto_reset = 0;
    a.px = pos_x; a.py = pos_y; a.vx = vel_x; a.vy = vel_y; a.act = act;
    return launch_step(a, (hipStream_t)stream);
}

int fg_observe_hd(const FgParams* params, int B, int N,
                  const float* pos_x, const float* pos_y, const float* vel_x, const float* vel_y,
                  const float* ideal_shape, const float* ideal_vel, const int32_t* step,
                  float* obs, float* reward, float* indiv_reward, uint8_t* done,
                  int32_t* near_lm, int32_t* near_ag, int32_t* hd_idx, void* stream) {
    const DeviceGuard device_guard(stream, pos_x);
    int rc = check_params(params);
    if (rc) return rc;
    if (B == 0) return FG_OK;                         // an empty batch is a no-op (e.g. a rank that owns no envs)
    if (B < 0) return fail(FG_ERR_BAD_ARG, "B must be >= 0%s");
    if ((rc = hd_n_check(N))) return rc;
    if (!pos_x || !pos_y || !vel_x || !vel_y || !ideal_shape || !ideal_vel) return null_pointer("fg_observe_hd");
    if (!obs && !reward) return fail(FG_ERR_BAD_ARG, "fg_observe_hd: obs and reward both NULL%s");
    if (((uintptr_t)obs & 15u) || ((uintptr_t)ideal_shape & 7u) || ((uintptr_t)ideal_vel & 7u))
        return fail(FG_ERR_ALIGNMENT, "obs must be 16-byte, ideal_shape/ideal_vel 8-byte aligned%s");
    Args a;
    if ((rc = hd_args(&a, params, B, N, 1, 1, 0, 1))) return rc;
    a.p.auto_reset = 0;
    hd_buffers(&a, const_cast<float*>(pos_x), const_cast<float*>(pos_y), const_cast<float*>(vel_x), const_cast<float*>(vel_y),
               const_cast<float*>(ideal_shape), const_cast<float*>(ideal_vel), const_cast<int32_t*>(step), obs, reward,
               indiv_reward, done);
    a.near_lm = near_lm; a.near_ag = near_ag; a.hd_idx = hd_idx;
    return launch_step(a, (hipStream_t)stream);
}

int fg_rollout_hd(const FgParams* params, int B, int N, int K,
                  float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                  const float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                  float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq,
                  int obs_every, void* stream) {
    const DeviceGuard device_guard(stream, pos_x);
    int rc = check_params(params);
    if (rc) return rc;
    if (B == 0 || K == 0) return FG_OK;               // empty batch / zero steps: nothing to do
    if (B < 0 || K < 0) return fail(FG_ERR_BAD_ARG, "B and K must be >= 0%s");
    if ((rc = hd_n_check(N))) return rc;
    const HdRollout r = {pos_x, pos_y, vel_x, vel_y, const_cast<float*>(act_seq), ideal_shape, ideal_vel, step,
                         obs_seq, reward_seq, indiv_seq, done_seq};
    if ((rc = rollout_buffers_check("fg_rollout_hd", r))) return rc;
    Args a;
    if ((rc = hd_args(&a, params, B, N, K, obs_every, 1, 1))) return rc;
    hd_buffers(&a, r);
    a.act = act_seq;
    return rollout_hd_dispatch(a, (hipStream_t)stream);
}

int fg_rollout_hd_policy(const FgParams* params, int B, int N, int K, int per_layer,
                         float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                         float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                         float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq,
                         int obs_every, void* stream) {
    const DeviceGuard device_guard(stream, pos_x);
    int rc = check_params(params);
    if (rc) return rc;
    if (B == 0 || K == 0) return FG_OK;
    if (B < 0 || K < 0) return fail(FG_ERR_BAD_ARG, "B and K must be >= 0%s");
    if ((rc = hd_n_check(N))) return rc;
    FgPolicyLevels pl;
    if ((rc = policy_levels_check("fg_rollout_hd_policy", N, per_layer, &pl))) return rc;
    const HdRollout r = {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, obs_seq, reward_seq, indiv_seq, done_seq};
    if ((rc = rollout_buffers_check("fg_rollout_hd_policy", r))) return rc;
    Args a;
    if ((rc = hd_args(&a, params, B, N, K, obs_every, 1, 1))) return rc;
    hd_buffers(&a, r);
    a.pl = pl; a.act_out = act_seq;
    return rollout_hd_policy_dispatch(a, per_layer, (hipStream_t)stream);
}

int fg_reset_hd(const FgParams* params, int B, int N, const uint8_t* mask,
                float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                float* ideal_shape, float* ideal_vel, int32_t* step, void* stream) {
    const DeviceGuard device_guard(stream, pos_x);
    int rc = check_params(params);
    if (rc) return rc;
    if (B == 0) return FG_OK;                         // an empty batch is a no-op (e.g. a rank that owns no envs)
    if (B < 0) return fail(FG_ERR_BAD_ARG, "B must be >= 0%s");
    if ((rc = generic_n_check(N))) return rc;
    if (!pos_x || !pos_y || !vel_x || !vel_y || !ideal_shape || !ideal_vel) return null_pointer("fg_reset_hd");
    Geometry g;
    geometry_for(N, &g);
    // (no hd_args: a reset writes no observation and does not look at the observation pitch)
    Args a; memset(&a, 0, sizeof(a));
    a.p = *params; a.B = B; a.N = N; a.inv_n = 1.0f / (float)N;
    hd_buffers(&a, pos_x, pos_y, vel_x, vel_y, ideal_shape, ideal_vel, step, nullptr, nullptr, nullptr, nullptr);
    return pow2_dispatch(g.G, [&](auto lanes, auto threads) {
        constexpr int GG = decltype(lanes)::value, TT = decltype(threads)::value;
        return launch<&reset_kernel<GG, TT>>((B + (TT / GG) - 1) / (TT / GG), TT, 0, (hipStream_t)stream, "reset launch failed: %s", a, mask);
    });
}

int fg_reset_hd_mt(int B, int N, const uint8_t* mask, uint32_t* mt_state,
                   float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                   float* ideal_shape, float* ideal_vel, float* landmark_pos, int32_t* step, void* stream) {
    return launch_mt_reset(B, N, mask, mt_state, pos_x, pos_y, vel_x, vel_y, ideal_shape, ideal_vel, landmark_pos, step,
                           0, nullptr, 0, stream);
}

int fg_reset_hd_mt_done(int B, int N, int world_length, uint32_t* mt_state,
                        float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                        float* ideal_shape, float* ideal_vel, float* landmark_pos, int32_t* step,
                        float* obs, int64_t obs_env_pitch, void* stream) {
    if (B == 0) return FG_OK;
    if (world_length <= 0 || !step) return fail(FG_ERR_BAD_ARG, "fg_reset_hd_mt_done: world_length > 0 and step required%s");
    return launch_mt_reset(B, N, nullptr, mt_state, pos_x, pos_y, vel_x, vel_y, ideal_shape, ideal_vel, landmark_pos, step,
                           world_length, obs, (long long)obs_env_pitch, stream);
}

int fg_reset_scenario(const FgParams* params, const FgScenario* scenario, int B, int N, const uint8_t* mask,
                      float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                      float* landmarks, float* obst_pos, float* obst_vel, int32_t* step, void* stream) {
    const DeviceGuard device_guard(stream, pos_x);
    int rc = check_params(params);
    if (rc || (rc = scn_given(scenario)) || (rc = scn_kind_check(scenario))) return rc;
    if (B == 0) return FG_OK;
    if ((rc = scn_counts_check(scenario, B, N))) return rc;
    if (scn_world_null(scenario, pos_x, pos_y, vel_x, vel_y, landmarks, obst_pos, obst_vel)) return null_pointer("fg_reset_scenario");
    if ((rc = scn_reset_align_check(landmarks, obst_pos, obst_vel))) return rc;
    const long long count = (long long)B * (N + scenario->num_landmarks + scenario->num_obstacles);
    return launch<&scn_reset_kernel>((unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream, "scenario reset launch failed: %s",
                                     *params, *scenario, B, N, mask, pos_x, pos_y, vel_x, vel_y, reinterpret_cast<float2*>(landmarks),
                                     reinterpret_cast<float2*>(obst_pos), reinterpret_cast<float2*>(obst_vel), step);
}

int fg_reset_scenario_mt(const FgScenario* scenario, int B, int N, const uint8_t* mask, int world_length, uint32_t* mt_state,
                         float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                         float* landmarks, float* obst_pos, float* obst_vel, int32_t* step, void* stream) {
    const DeviceGuard device_guard(stream, pos_x);
    int rc = scn_given(scenario);                     // (no kind check: the MT19937 reset draws the same for every kind)
    if (rc) return rc;
    if (B == 0) return FG_OK;
    if ((rc = scn_counts_check(scenario, B, N))) return rc;
    if (!mt_state || scn_world_null(scenario, pos_x, pos_y, vel_x, vel_y, landmarks, obst_pos, obst_vel))
        return null_pointer("fg_reset_scenario_mt");
    if (!mask && world_length > 0 && !step) return fail(FG_ERR_BAD_ARG, "fg_reset_scenario_mt: the done rule needs the step counters%s");
    if ((rc = scn_reset_align_check(landmarks, obst_pos, obst_vel))) return rc;
    const int L = scenario->num_landmarks, M = scenario->num_obstacles;
    const int lds = (624 + 4 * (N + L + M)) * (int)sizeof(uint32_t);
    return launch<&mt_reset_scn_kernel>(B, 256, lds, (hipStream_t)stream, "mt reset launch failed: %s", B, N, L, M, mask, mt_state,
                                        pos_x, pos_y, vel_x, vel_y, reinterpret_cast<float2*>(landmarks),
                                        reinterpret_cast<float2*>(obst_pos), reinterpret_cast<float2*>(obst_vel), step, world_length,
                                        scenario->obstacle_vx, scenario->obstacle_vy);
}

int fg_update_comm(const FgParams* params, int B, int N, const float* action_c, float* comm_state, void* stream) {
    const DeviceGuard device_guard(stream, comm_state);
    int rc = check_params(params);
    if (rc) return rc;
    if (B == 0) return FG_OK;
    if (B < 0) return fail(FG_ERR_BAD_ARG, "B must be >= 0%s");
    if (N < 1 || N > FG_MAX_AGENTS) return fail(FG_ERR_UNSUPPORTED_N, "N must be in [1, 1024]%s");
    if (!action_c || !comm_state) return null_pointer("fg_update_comm");
    if (((uintptr_t)action_c & 7u) || ((uintptr_t)comm_state & 7u))
        return fail(FG_ERR_ALIGNMENT, "action_c and comm_state must be 8-byte aligned%s");
    const long long count = (long long)B * N;
    return launch<&update_comm_kernel>((unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream, "comm launch failed: %s", *params,
                                       B, N, reinterpret_cast<const float2*>(action_c), reinterpret_cast<float2*>(comm_state));
}

int fg_update_comm_dim(const FgParams* params, int B, int N, int dim_c, const float* action_c, float* comm_state, void* stream) {
    if (dim_c == 2) return fg_update_comm(params, B, N, action_c, comm_state, stream);
    const DeviceGuard device_guard(stream, comm_state);
    int rc = check_params(params);
    if (rc) return rc;
    if (B == 0 || dim_c == 0) return FG_OK;
    if (B < 0 || dim_c < 0 || dim_c > 4096) return fail(FG_ERR_BAD_ARG, "B >= 0 and 0 <= dim_c <= 4096 required%s");
    if (N < 1 || N > FG_MAX_AGENTS) return fail(FG_ERR_UNSUPPORTED_N, "N must be in [1, 1024]%s");
    if (!action_c || !comm_state) return null_pointer("fg_update_comm_dim");
    if (((uintptr_t)action_c & 3u) || ((uintptr_t)comm_state & 3u))
        return fail(FG_ERR_ALIGNMENT, "action_c and comm_state must be 4-byte aligned%s");
    const long long count = (long long)B * N * ((dim_c + 1) / 2);
    return launch<&update_comm_dim_kernel>((unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream, "comm launch failed: %s",
                                           *params, B, N, dim_c, action_c, comm_state);
}

int fg_step_scenario(const FgParams* params, const FgScenario* scenario, int B, int N, int do_physics,
                     float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                     const float* act, float* landmarks, float* obst_pos, float* obst_vel,
                     int32_t* step, float* obs, float* reward, float* indiv_reward, uint8_t* done,
                     void* stream) {
    return launch_scenario(params, scenario, B, N, do_physics, 1, 1,
                           scn_buffers(pos_x, pos_y, vel_x, vel_y, act, landmarks, obst_pos, obst_vel, step, obs, reward,
                                       indiv_reward, done, nullptr), stream);
}

int fg_step_basic(const FgParams* params, int B, int N, int L, int do_physics,
                  float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                  const float* act, float* landmarks, int32_t* step,
                  float* obs, float* reward, float* indiv_reward, uint8_t* done,
                  int32_t* near_ag, void* stream) {
    FgScenario sc; memset(&sc, 0, sizeof(sc));
    sc.kind = FG_SCN_BASIC; sc.num_landmarks = L; sc.penalty = 1.0f;
    return launch_scenario(params, &sc, B, N, do_physics, 1, 1,
                           scn_buffers(pos_x, pos_y, vel_x, vel_y, act, landmarks, nullptr, nullptr, step, obs, reward,
                                       indiv_reward, done, near_ag), stream);
}

int fg_rollout_scenario(const FgParams* params, const FgScenario* scenario, int B, int N, int K,
                        float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                        const float* act_seq, float* landmarks, float* obst_pos, float* obst_vel,
                        int32_t* step, float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq,
                        int32_t* near_ag_seq, int obs_every, void* stream) {
    return launch_scenario(params, scenario, B, N, 1, K, obs_every < 1 ? 1 : obs_every,
                           scn_buffers(pos_x, pos_y, vel_x, vel_y, act_seq, landmarks, obst_pos, obst_vel, step, obs_seq,
                                       reward_seq, indiv_seq, done_seq, near_ag_seq), stream);
}

int fg_policy_bfs_state(int B, int N, int per_layer, const float* pos_x, const float* pos_y,
                        const float* ideal_shape, const float* ideal_vel, float* act, void* stream) {
    const DeviceGuard device_guard(stream, pos_x);
    if (B == 0) return FG_OK;
    if (B < 0) return fail(FG_ERR_BAD_ARG, "B must be >= 0%s");
    int rc = hd_n_check(N);
    if (rc) return rc;
    FgPolicyLevels pl;
    if ((rc = policy_levels_check("fg_policy_bfs_state", N, per_layer, &pl))) return rc;
    if (!pos_x || !pos_y || !ideal_shape || !ideal_vel || !act) return null_pointer("fg_policy_bfs_state");
    if (((uintptr_t)ideal_shape & 7u) || ((uintptr_t)ideal_vel & 7u) || ((uintptr_t)act & 7u))
        return fail(FG_ERR_ALIGNMENT, "ideal_shape, ideal_vel and act must be 8-byte aligned%s");
    return launch_policy_state(B, N, pl, pos_x, pos_y, ideal_shape, ideal_vel, act, (hipStream_t)stream);
}

int fg_policy_bfs(int B, int N, int per_layer, const float* obs, int64_t obs_env_stride, float* act, void* stream) {
    const DeviceGuard device_guard(stream, act);    // the actions (obs may live in an fg_arena, whose pointers carry no device attribute on every runtime)
    if (B == 0) return FG_OK;
    if (B < 0) return fail(FG_ERR_BAD_ARG, "B must be >= 0%s");
    int rc = hd_n_check(N);
    if (rc) return rc;
    FgPolicyLevels pl;
    if ((rc = policy_levels_check("fg_policy_bfs", N, per_layer, &pl))) return rc;
    if (!obs || !act) return null_pointer("fg_policy_bfs");
    const int64_t stride = obs_env_stride ? obs_env_stride : 6LL * N * N;
    if (stride < 6LL * N || (stride & 1)) return fail(FG_ERR_BAD_ARG, "fg_policy_bfs: obs_env_stride must be even and >= 6 N%s");
    if (((uintptr_t)obs & 7u) || ((uintptr_t)act & 7u)) return fail(FG_ERR_ALIGNMENT, "obs and act must be 8-byte aligned%s");
    const PolicyGeometry g = policy_geometry(B, N);
    return policy_per_dispatch(per_layer, [&](auto per) {
        return launch<&policy_bfs_kernel<decltype(per)::value>>(g.grid, 256, g.lds, (hipStream_t)stream, "policy launch failed: %s", B, N,
                                                                g.lpe, pl, obs, (long long)stride, act);
    });
}

int fg_decode_actions(int mode, int64_t count, void* action, float* u_out, void* stream) {
    const DeviceGuard device_guard(stream, u_out);
    if (mode != FG_ACT_ONEHOT5 && mode != FG_ACT_INDEX && mode != FG_ACT_ARGMAX)
        return fail(FG_ERR_BAD_ARG, "fg_decode_actions: unknown mode%s");
    if (count == 0) return FG_OK;
    if (count < 0 || count > ((int64_t)1 << 38)) return fail(FG_ERR_BAD_ARG, "fg_decode_actions: count out of range%s");
    if (!action || !u_out) return null_pointer("fg_decode_actions");
    if (((uintptr_t)u_out & 7) || (mode == FG_ACT_ARGMAX && ((uintptr_t)action & 7)))
        return fail(FG_ERR_ALIGNMENT, "fg_decode_actions: buffers must be 8-byte aligned%s");
    return launch<&decode_actions_kernel>((unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream, "decode launch failed: %s",
                                          mode, count, action, reinterpret_cast<float2*>(u_out));
}

// ---- closed loop with the caller's MLP actor ----
int fg_rollout_hd_actor(const FgParams* params, const FgActor* actor, int B, int N, int K,
                        float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                        float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                        float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq,
                        int obs_every, void* stream) {
    return rollout_actor_impl(params, {HD_ACTOR_SHARED, actor}, B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, obs_seq, reward_seq, indiv_seq,
                               done_seq}, obs_every, stream);
}

int fg_rollout_hd_actor_sample(const FgParams* params, const FgActor* actor, const float* log_std, int B, int N, int K,
                               float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                               float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                               float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                               int obs_every, void* stream) {
    return rollout_actor_impl(params, {HD_ACTOR_SAMPLE, actor, log_std, logp_seq}, B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, obs_seq, reward_seq, indiv_seq,
                               done_seq}, obs_every, stream);
}

int fg_rollout_hd_actor_per_agent(const FgParams* params, const FgActor* actors, const float* log_std, int B, int N, int K,
                                  float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                                  float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                                  float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                                  int obs_every, void* stream) {
    return rollout_actor_impl(params, {HD_ACTOR_PER_AGENT, actors, log_std, logp_seq}, B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, obs_seq, reward_seq, indiv_seq,
                               done_seq}, obs_every, stream);
}

int fg_rollout_hd_actor_norm(const FgParams* params, const FgActor* actor, const FgActorNorm* norm, const float* log_std,
                             int B, int N, int K, float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                             float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                             float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                             int obs_every, void* stream) {
    return rollout_actor_impl(params, {HD_ACTOR_NORM, actor, log_std, logp_seq, nullptr, norm}, B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, obs_seq, reward_seq, indiv_seq,
                               done_seq}, obs_every, stream);
}

int fg_rollout_hd_actor_gru(const FgParams* params, const FgActor* actor, const FgActorNorm* norm, const FgActorGru* gru,
                            const float* log_std, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                            float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                            float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                            float* rnn_state, int obs_every, void* stream) {
    return rollout_actor_impl(params, {HD_ACTOR_GRU, actor, log_std, logp_seq, nullptr, norm, gru, rnn_state}, B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, obs_seq, reward_seq, indiv_seq,
                               done_seq}, obs_every, stream);
}

int fg_rollout_hd_actor_gru_states(const FgParams* params, const FgActor* actor, const FgActorNorm* norm, const FgActorGru* gru,
                                   const float* log_std, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x,
                                   float* vel_y, float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                                   float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                                   float* rnn_state, float* rnn_states, int states_every, int obs_every, void* stream) {
    return rollout_actor_impl(params,
                              {HD_ACTOR_GRU, actor, log_std, logp_seq, nullptr, norm, gru, rnn_state, true, rnn_states, states_every}, B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, obs_seq, reward_seq, indiv_seq,
                               done_seq}, obs_every, stream);
}

int fg_rollout_hd_actor_bn(const FgParams* params, const FgActor* actor, const FgActorInBn* in_bn, const float* log_std,
                           int B, int N, int K, float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                           float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                           float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                           int obs_every, void* stream) {
    return rollout_actor_impl(params, {HD_ACTOR_BN, actor, log_std, logp_seq, in_bn}, B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, obs_seq, reward_seq, indiv_seq,
                               done_seq}, obs_every, stream);
}

int fg_rollout_hd_actor_bn_per_agent(const FgParams* params, const FgActor* actors, const FgActorInBn* in_bns,
                                     const float* log_std, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x,
                                     float* vel_y, float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                                     float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                                     int obs_every, void* stream) {
    return rollout_actor_impl(params, {HD_ACTOR_BN_PER_AGENT, actors, log_std, logp_seq, in_bns}, B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, obs_seq, reward_seq, indiv_seq,
                               done_seq}, obs_every, stream);
}

// the OU entries' call: the inner actor's family with `noise` set (no log_std, no logp)
static HdActorCall hd_actor_ou_call(bool members, const FgActor* actor, const FgActorInBn* in_bn, const FgActorOu* ou, float* state) {
    HdActorCall c{members ? (in_bn ? HD_ACTOR_BN_PER_AGENT : HD_ACTOR_PER_AGENT) : (in_bn ? HD_ACTOR_BN : HD_ACTOR_SHARED), actor};
    c.in_bn = in_bn;
    c.noise = {true, ou, state};
    return c;
}

int fg_rollout_hd_actor_ou(const FgParams* params, const FgActor* actor, const FgActorInBn* in_bn, const FgActorOu* ou,
                           float* noise_state, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                           float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                           float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, int obs_every, void* stream) {
    return rollout_actor_impl(params, hd_actor_ou_call(false, actor, in_bn, ou, noise_state), B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, obs_seq, reward_seq, indiv_seq,
                               done_seq}, obs_every, stream);
}

int fg_rollout_hd_actor_ou_per_agent(const FgParams* params, const FgActor* actors, const FgActorInBn* in_bns, const FgActorOu* ou,
                                     float* noise_state, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x,
                                     float* vel_y, float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                                     float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, int obs_every,
                                     void* stream) {
    return rollout_actor_impl(params, hd_actor_ou_call(true, actors, in_bns, ou, noise_state), B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, obs_seq, reward_seq, indiv_seq,
                               done_seq}, obs_every, stream);
}

// the Gumbel entries' call: the logits' family with `gumbel` set (no log_std, no logp)
static HdActorCall hd_actor_gumbel_call(bool members, const FgActor* actor, const FgActorInBn* in_bn, int act_mode, int explore,
                                        int32_t* idx) {
    HdActorCall c{members ? (in_bn ? HD_ACTOR_BN_PER_AGENT : HD_ACTOR_PER_AGENT) : (in_bn ? HD_ACTOR_BN : HD_ACTOR_SHARED), actor};
    c.in_bn = in_bn;
    c.gumbel = {true, act_mode, explore, idx};
    return c;
}

int fg_rollout_hd_actor_gumbel(const FgParams* params, const FgActor* actor, const FgActorInBn* in_bn, int act_mode, int explore,
                               int B, int N, int K, float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                               float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                               float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, int32_t* idx_seq,
                               int obs_every, void* stream) {
    return rollout_actor_impl(params, hd_actor_gumbel_call(false, actor, in_bn, act_mode, explore, idx_seq), B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, obs_seq, reward_seq, indiv_seq,
                               done_seq}, obs_every, stream);
}

int fg_rollout_hd_actor_gumbel_per_agent(const FgParams* params, const FgActor* actors, const FgActorInBn* in_bns, int act_mode,
                                         int explore, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x,
                                         float* vel_y, float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                                         float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, int32_t* idx_seq,
                                         int obs_every, void* stream) {
    return rollout_actor_impl(params, hd_actor_gumbel_call(true, actors, in_bns, act_mode, explore, idx_seq), B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, obs_seq, reward_seq, indiv_seq,
                               done_seq}, obs_every, stream);
}

// the categorical entries' call: the body's family - recurrent with `gru`, LayerNorm with `norm` alone, else shared - with `cat`
// set (no log_std); `rnn_states` NULL: no record of the states.  A `gru` without `norm` fails the recurrent family's own check
// of its norms (FG_ERR_BAD_ARG, "norm is NULL").
static HdActorCall hd_actor_cat_call(const FgActor* actor, const FgActorNorm* norm, const FgActorGru* gru, int act_mode, int greedy,
                                     int32_t* idx, float* logp, float* rnn_state, float* rnn_states, int states_every) {
    HdActorCall c{gru ? HD_ACTOR_GRU : norm ? HD_ACTOR_NORM : HD_ACTOR_SHARED, actor};
    c.norm = norm;
    c.gru = gru;
    c.rnn_state = rnn_state;
    if (gru && rnn_states) { c.states_entry = true; c.rnn_states = rnn_states; c.states_every = states_every; }
    c.cat = {true, act_mode, greedy, idx, logp};
    return c;
}

int fg_rollout_hd_actor_cat(const FgParams* params, const FgActor* actor, const FgActorNorm* norm, const FgActorGru* gru,
                            int act_mode, int greedy, int B, int N, int K, float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                            float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                            float* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, int32_t* idx_seq,
                            float* logp_seq, float* rnn_state, float* rnn_states, int states_every, int obs_every, void* stream) {
    return rollout_actor_impl(params, hd_actor_cat_call(actor, norm, gru, act_mode, greedy, idx_seq, logp_seq, rnn_state, rnn_states,
                                                        states_every), B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, obs_seq, reward_seq, indiv_seq,
                               done_seq}, obs_every, stream);
}

// the 16-bit entries' call: the Gaussian (`log_std`, required) or categorical call of the body's family with `obs_format` set
static HdActorCall hd_actor_obs16_call(HdActorCall c, int obs_format) {
    c.obs_format = (obs_format == FG_OBS_F16 || obs_format == FG_OBS_BF16) ? obs_format : -1;
    return c;
}
static HdActorCall hd_actor_gauss_call(const FgActor* actor, const FgActorNorm* norm, const FgActorGru* gru, const float* log_std,
                                       float* logp, float* rnn_state, float* rnn_states, int states_every) {
    HdActorCall c{gru ? HD_ACTOR_GRU : norm ? HD_ACTOR_NORM : HD_ACTOR_SAMPLE, actor, log_std, logp};
    c.norm = norm;
    c.gru = gru;
    c.rnn_state = rnn_state;
    if (gru && rnn_states) { c.states_entry = true; c.rnn_states = rnn_states; c.states_every = states_every; }
    return c;
}

int fg_rollout_hd_actor_obs16(const FgParams* params, int obs_format, const FgActor* actor, const FgActorNorm* norm,
                              const FgActorGru* gru, const float* log_std, int B, int N, int K, float* pos_x, float* pos_y,
                              float* vel_x, float* vel_y, float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                              void* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, float* logp_seq,
                              float* rnn_state, float* rnn_states, int states_every, int obs_every, void* stream) {
    return rollout_actor_impl(params, hd_actor_obs16_call(hd_actor_gauss_call(actor, norm, gru, log_std, logp_seq, rnn_state, rnn_states,
                                                                              states_every), obs_format), B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, static_cast<float*>(obs_seq), reward_seq,
                               indiv_seq, done_seq}, obs_every, stream);
}

int fg_rollout_hd_actor_cat_obs16(const FgParams* params, int obs_format, const FgActor* actor, const FgActorNorm* norm,
                                  const FgActorGru* gru, int act_mode, int greedy, int B, int N, int K, float* pos_x, float* pos_y,
                                  float* vel_x, float* vel_y, float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                                  void* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq, int32_t* idx_seq,
                                  float* logp_seq, float* rnn_state, float* rnn_states, int states_every, int obs_every,
                                  void* stream) {
    return rollout_actor_impl(params, hd_actor_obs16_call(hd_actor_cat_call(actor, norm, gru, act_mode, greedy, idx_seq, logp_seq,
                                                                            rnn_state, rnn_states, states_every), obs_format), B, N, K,
                              {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step, static_cast<float*>(obs_seq), reward_seq,
                               indiv_seq, done_seq}, obs_every, stream);
}

int fg_actor_uniform(const FgParams* params, int B, int N, float* u, void* stream) {
    int rc = check_params(params);
    if (rc) return rc;
    if (B < 0 || N < 1 || N >= (1 << 29)) return fail(FG_ERR_BAD_ARG, "fg_actor_uniform: B >= 0 and 1 <= N < 2^29 required%s");
    if (!u) return fail(FG_ERR_BAD_ARG, "fg_actor_uniform: u is NULL%s");
    if ((uintptr_t)u & 3u) return fail(FG_ERR_ALIGNMENT, "fg_actor_uniform: u must be 4-byte aligned%s");
    if (B == 0) return FG_OK;
    const DeviceGuard device_guard(stream, u);
    const long long count = (long long)B * N;
    return launch<&actor_uniform_kernel>((unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream,
                                         "actor uniform launch failed: %s", *params, B, N, u);
}

int fg_actor_categorical(int act_mode, int greedy, int64_t count, const float* logits, const float* u, int32_t* idx, float* act,
                         float* logp, void* stream) {
    if (act_mode != FG_ACT_ONEHOT5 && act_mode != FG_ACT_INDEX)
        return fail(FG_ERR_BAD_ARG, "fg_actor_categorical: act_mode must be FG_ACT_ONEHOT5 or FG_ACT_INDEX%s");
    if (count < 0 || count > ((int64_t)1 << 38)) return fail(FG_ERR_BAD_ARG, "fg_actor_categorical: count out of range%s");
    if (count == 0) return FG_OK;
    if (!logits || !idx || (!u && !greedy)) return fail(FG_ERR_BAD_ARG, "fg_actor_categorical: logits, idx and (sampling) u are required%s");
    if ((((uintptr_t)logits | (uintptr_t)u | (uintptr_t)idx | (uintptr_t)logp) & 3u) || ((uintptr_t)act & 7u))
        return fail(FG_ERR_ALIGNMENT, "fg_actor_categorical: act must be 8-byte, the other buffers 4-byte aligned%s");
    const DeviceGuard device_guard(stream, idx);
    return launch<&actor_categorical_kernel>((unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream,
                                             "actor categorical launch failed: %s", act_mode, greedy ? 1 : 0, (long long)count, logits, u,
                                             reinterpret_cast<int*>(idx), reinterpret_cast<float2*>(act), logp);
}

int fg_actor_gumbel(const FgParams* params, int B, int N, float* g, void* stream) {
    int rc = check_params(params);
    if (rc) return rc;
    if (B < 0 || N < 1 || N > (1 << 12)) return fail(FG_ERR_BAD_ARG, "fg_actor_gumbel: B >= 0 and 1 <= N <= 2^12 required%s");
    if (!g) return fail(FG_ERR_BAD_ARG, "fg_actor_gumbel: g is NULL%s");
    if ((uintptr_t)g & 3u) return fail(FG_ERR_ALIGNMENT, "fg_actor_gumbel: g must be 4-byte aligned%s");
    if (B == 0) return FG_OK;
    const DeviceGuard device_guard(stream, g);
    const long long count = (long long)B * N;
    return launch<&actor_gumbel_kernel>((unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream,
                                        "actor gumbel launch failed: %s", *params, B, N, g);
}

int fg_actor_gumbel_pick(int act_mode, int explore, int64_t count, const float* logits, const float* g, int32_t* idx, float* act,
                         void* stream) {
    if (act_mode != FG_ACT_ONEHOT5 && act_mode != FG_ACT_INDEX)
        return fail(FG_ERR_BAD_ARG, "fg_actor_gumbel_pick: act_mode must be FG_ACT_ONEHOT5 or FG_ACT_INDEX%s");
    if (count < 0 || count > ((int64_t)1 << 38)) return fail(FG_ERR_BAD_ARG, "fg_actor_gumbel_pick: count out of range%s");
    if (count == 0) return FG_OK;
    if (!logits || !idx || (!g && explore)) return fail(FG_ERR_BAD_ARG, "fg_actor_gumbel_pick: logits, idx and (exploring) g are required%s");
    if ((((uintptr_t)logits | (uintptr_t)g | (uintptr_t)idx) & 3u) || ((uintptr_t)act & 7u))
        return fail(FG_ERR_ALIGNMENT, "fg_actor_gumbel_pick: act must be 8-byte, the other buffers 4-byte aligned%s");
    const DeviceGuard device_guard(stream, idx);
    return launch<&actor_gumbel_pick_kernel>((unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream,
                                             "actor gumbel pick launch failed: %s", act_mode, explore ? 1 : 0, (long long)count, logits, g,
                                             reinterpret_cast<int*>(idx), reinterpret_cast<float2*>(act));
}

int fg_actor_ou_step(const FgActorOu* ou, int64_t count, const float* eps, float* state, void* stream) {
    if (count < 0) return fail(FG_ERR_BAD_ARG, "fg_actor_ou_step: count >= 0 required%s");
    const int rc = actor_ou_check("fg_actor_ou_step", ou, state, count > 0 ? 1 : 0);
    if (rc) return rc;
    if (count == 0) return FG_OK;
    if (!eps) return fail(FG_ERR_BAD_ARG, "fg_actor_ou_step: eps is NULL%s");
    if ((uintptr_t)eps & 7u) return fail(FG_ERR_ALIGNMENT, "fg_actor_ou_step: eps must be 8-byte aligned%s");
    const DeviceGuard device_guard(stream, state);
    return launch<&actor_ou_step_kernel>((unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream, "actor OU step launch failed: %s",
                                         (long long)count, ou->theta, ou->mu, ou->sigma, reinterpret_cast<const float2*>(eps),
                                         reinterpret_cast<float2*>(state));
}

int fg_actor_noise(const FgParams* params, int B, int N, float* eps, void* stream) {
    int rc = check_params(params);
    if (rc) return rc;
    if (B < 0 || N < 1 || N >= (1 << 29)) return fail(FG_ERR_BAD_ARG, "fg_actor_noise: B >= 0 and 1 <= N < 2^29 required%s");
    if (!eps) return fail(FG_ERR_BAD_ARG, "fg_actor_noise: eps is NULL%s");
    if ((uintptr_t)eps & 7u) return fail(FG_ERR_ALIGNMENT, "fg_actor_noise: eps must be 8-byte aligned%s");
    if (B == 0) return FG_OK;
    const DeviceGuard device_guard(stream, eps);
    const long long count = (long long)B * N;
    return launch<&actor_noise_kernel>((unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream, "actor noise launch failed: %s",
                                       *params, B, N, reinterpret_cast<float2*>(eps));
}

int fg_actor_log_prob(const float* eps, const float* log_std, int64_t count, float* logp, void* stream) {
    if (count < 0) return fail(FG_ERR_BAD_ARG, "fg_actor_log_prob: count >= 0 required%s");
    if (count == 0) return FG_OK;
    if (!eps || !log_std || !logp) return fail(FG_ERR_BAD_ARG, "fg_actor_log_prob: eps, log_std and logp are required%s");
    if (((uintptr_t)eps & 7u) || (((uintptr_t)log_std | (uintptr_t)logp) & 3u))
        return fail(FG_ERR_ALIGNMENT, "fg_actor_log_prob: eps must be 8-byte, log_std and logp 4-byte aligned%s");
    const DeviceGuard device_guard(stream, eps);
    return launch<&actor_logp_kernel>((unsigned)((count + 255) / 256), 256, 0, (hipStream_t)stream, "actor log-prob launch failed: %s",
                                      (long long)count, reinterpret_cast<const float2*>(eps), log_std, logp);
}

int fg_describe_actor_launch(const FgParams* params, const FgActor* actor, int B, int N, int K, int obs_every,
                             char* out, int out_len) {
    return describe_actor_impl("fg_describe_actor_launch", params, {HD_ACTOR_SHARED, actor},
                               B, N, K, obs_every, out, out_len);
}

int fg_describe_actor_sample_launch(const FgParams* params, const FgActor* actor, const float* log_std, int B, int N, int K,
                                    int obs_every, char* out, int out_len) {
    return describe_actor_impl("fg_describe_actor_sample_launch", params, {HD_ACTOR_SAMPLE, actor, log_std},
                               B, N, K, obs_every, out, out_len);
}

int fg_describe_actor_norm_launch(const FgParams* params, const FgActor* actor, const FgActorNorm* norm, const float* log_std,
                                  int B, int N, int K, int obs_every, char* out, int out_len) {
    return describe_actor_impl("fg_describe_actor_norm_launch", params, {HD_ACTOR_NORM, actor, log_std, nullptr, nullptr, norm},
                               B, N, K, obs_every, out, out_len);
}

int fg_describe_actor_gru_launch(const FgParams* params, const FgActor* actor, const FgActorNorm* norm, const FgActorGru* gru,
                                 const float* log_std, int B, int N, int K, int obs_every, char* out, int out_len) {
    float* const state = reinterpret_cast<float*>((uintptr_t)4096);      // a stand-in: the dry run has no hidden state
    return describe_actor_impl("fg_describe_actor_gru_launch", params, {HD_ACTOR_GRU, actor, log_std, nullptr, nullptr, norm, gru, state},
                               B, N, K, obs_every, out, out_len);
}

int fg_describe_actor_per_agent_launch(const FgParams* params, const FgActor* actors, const float* log_std, int B, int N,
                                      int K, int obs_every, char* out, int out_len) {
    return describe_actor_impl("fg_describe_actor_per_agent_launch", params, {HD_ACTOR_PER_AGENT, actors, log_std},
                               B, N, K, obs_every, out, out_len);
}

int fg_describe_actor_bn_launch(const FgParams* params, const FgActor* actor, const FgActorInBn* in_bn, const float* log_std,
                                int B, int N, int K, int obs_every, char* out, int out_len) {
    return describe_actor_impl("fg_describe_actor_bn_launch", params, {HD_ACTOR_BN, actor, log_std, nullptr, in_bn},
                               B, N, K, obs_every, out, out_len);
}

int fg_describe_actor_bn_per_agent_launch(const FgParams* params, const FgActor* actors, const FgActorInBn* in_bns,
                                          const float* log_std, int B, int N, int K, int obs_every, char* out, int out_len) {
    return describe_actor_impl("fg_describe_actor_bn_per_agent_launch", params, {HD_ACTOR_BN_PER_AGENT, actors, log_std, nullptr, in_bns},
                               B, N, K, obs_every, out, out_len);
}

int fg_describe_actor_ou_launch(const FgParams* params, const FgActor* actor, const FgActorInBn* in_bn, const FgActorOu* ou,
                                int B, int N, int K, int obs_every, char* out, int out_len) {
    float* const state = reinterpret_cast<float*>((uintptr_t)4096);      // a stand-in: the dry run has no noise state
    return describe_actor_impl("fg_describe_actor_ou_launch", params, hd_actor_ou_call(false, actor, in_bn, ou, state),
                               B, N, K, obs_every, out, out_len);
}

int fg_describe_actor_ou_per_agent_launch(const FgParams* params, const FgActor* actors, const FgActorInBn* in_bns,
                                          const FgActorOu* ou, int B, int N, int K, int obs_every, char* out, int out_len) {
    float* const state = reinterpret_cast<float*>((uintptr_t)4096);
    return describe_actor_impl("fg_describe_actor_ou_per_agent_launch", params, hd_actor_ou_call(true, actors, in_bns, ou, state),
                               B, N, K, obs_every, out, out_len);
}

int fg_describe_actor_gumbel_launch(const FgParams* params, const FgActor* actor, const FgActorInBn* in_bn, int act_mode,
                                    int explore, int B, int N, int K, int obs_every, char* out, int out_len) {
    int32_t* const idx = reinterpret_cast<int32_t*>((uintptr_t)4096);   // a stand-in: the dry run has no outputs
    return describe_actor_impl("fg_describe_actor_gumbel_launch", params,
                               hd_actor_gumbel_call(false, actor, in_bn, act_mode, explore, idx), B, N, K, obs_every, out, out_len);
}

int fg_describe_actor_gumbel_per_agent_launch(const FgParams* params, const FgActor* actors, const FgActorInBn* in_bns,
                                              int act_mode, int explore, int B, int N, int K, int obs_every, char* out,
                                              int out_len) {
    int32_t* const idx = reinterpret_cast<int32_t*>((uintptr_t)4096);
    return describe_actor_impl("fg_describe_actor_gumbel_per_agent_launch", params,
                               hd_actor_gumbel_call(true, actors, in_bns, act_mode, explore, idx), B, N, K, obs_every, out, out_len);
}

int fg_describe_actor_cat_launch(const FgParams* params, const FgActor* actor, const FgActorNorm* norm, const FgActorGru* gru,
                                 int act_mode, int greedy, int B, int N, int K, int obs_every, char* out, int out_len) {
    float* const state = reinterpret_cast<float*>((uintptr_t)4096);      // stand-ins: the dry run has no state and no outputs
    int32_t* const idx = reinterpret_cast<int32_t*>((uintptr_t)4096);
    return describe_actor_impl("fg_describe_actor_cat_launch", params,
                               hd_actor_cat_call(actor, norm, gru, act_mode, greedy, idx, nullptr, state, nullptr, 1),
                               B, N, K, obs_every, out, out_len);
}

int fg_describe_actor_obs16_launch(const FgParams* params, int obs_format, const FgActor* actor, const FgActorNorm* norm,
                                   const FgActorGru* gru, const float* log_std, int B, int N, int K, int obs_every, char* out,
                                   int out_len) {
    float* const state = reinterpret_cast<float*>((uintptr_t)4096);      // a stand-in: the dry run has no hidden state
    return describe_actor_impl("fg_describe_actor_obs16_launch", params,
                               hd_actor_obs16_call(hd_actor_gauss_call(actor, norm, gru, log_std, nullptr, state, nullptr, 1), obs_format),
                               B, N, K, obs_every, out, out_len);
}

int fg_describe_actor_cat_obs16_launch(const FgParams* params, int obs_format, const FgActor* actor, const FgActorNorm* norm,
                                       const FgActorGru* gru, int act_mode, int greedy, int B, int N, int K, int obs_every,
                                       char* out, int out_len) {
    float* const state = reinterpret_cast<float*>((uintptr_t)4096);      // stand-ins: the dry run has no state and no outputs
    int32_t* const idx = reinterpret_cast<int32_t*>((uintptr_t)4096);
    return describe_actor_impl("fg_describe_actor_cat_obs16_launch", params,
                               hd_actor_obs16_call(hd_actor_cat_call(actor, norm, gru, act_mode, greedy, idx, nullptr, state, nullptr, 1),
                                                   obs_format),
                               B, N, K, obs_every, out, out_len);
}

int fg_rollout_scenario_actor(const FgParams* params, const FgScenario* scenario, const FgActor* actor, const float* log_std,
                              int B, int N, int K, float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                              float* landmarks, float* obst_pos, float* obst_vel, int32_t* step,
                              float* obs, float* reward, float* indiv_reward, uint8_t* done, float* act_out, float* logp,
                              int obs_every, void* stream) {
    int rc = scn_actor_check(params, scenario, actor, log_std, logp, B, N, K);
    if (rc) return rc;
    if (scn_world_null(scenario, pos_x, pos_y, vel_x, vel_y, landmarks, obst_pos, obst_vel) || !step || !reward || !act_out)
        return null_pointer("fg_rollout_scenario_actor");
    if (((uintptr_t)obs & 7u) || ((uintptr_t)landmarks & 7u) || ((uintptr_t)act_out & 7u) || ((uintptr_t)obst_pos & 7u) ||
        ((uintptr_t)obst_vel & 7u))
        return fail(FG_ERR_ALIGNMENT, "fg_rollout_scenario_actor: obs/landmarks/act_out/obstacle buffers must be 8-byte aligned%s");
    ScnArgs a = scn_buffers(pos_x, pos_y, vel_x, vel_y, nullptr, landmarks, obst_pos, obst_vel, step, obs, reward, indiv_reward,
                            done, nullptr);
    scn_args(&a, params, scenario, B, N, 1, K, obs_every);
    if (B == 0) {                                      // nothing to launch; an unsupported shape is still reported
        char dry[8];
        dry[0] = 0; a.B = 1;
        const DescribeScope describing(dry, (int)sizeof(dry));
        return scn_actor_dispatch(a, *actor, nullptr, log_std, nullptr, nullptr);
    }
    const DeviceGuard device_guard(stream, pos_x);
    return scn_actor_dispatch(a, *actor, act_out, log_std, logp, (hipStream_t)stream);
}

int fg_describe_scenario_actor_launch(const FgParams* params, const FgScenario* scenario, const FgActor* actor,
                                      const float* log_std, int B, int N, int K, int obs_every, char* out, int out_len) {
    if (!out || out_len < 2) return fail(FG_ERR_BAD_ARG, "fg_describe_scenario_actor_launch: out buffer required%s");
    out[0] = 0;
    int rc = scn_actor_check(params, scenario, actor, log_std, nullptr, B, N, K);
    if (rc) return rc;
    if (B <= 0) return fail(FG_ERR_BAD_ARG, "fg_describe_scenario_actor_launch: B > 0 required%s");
    ScnArgs a; memset(&a, 0, sizeof(a));
    scn_args(&a, params, scenario, B, N, 1, K, obs_every);
    const DescribeScope describing(out, out_len);
    return scn_actor_dispatch(a, *actor, nullptr, log_std, nullptr, nullptr);
}

// The dry run of fg_step_hd (K = 0), fg_rollout_hd (K steps), fg_rollout_hd_policy (per_layer > 0) or, with a scenario,
// fg_rollout_scenario: the entry's checks before its buffers, then its dispatch.  Nothing is dereferenced on the way; only the
// NULL-ness of the observation and index outputs steers the formation_hd_env dispatch, hence the stand-ins.
int fg_describe_launch(const FgParams* params, const FgScenario* scenario, int B, int N, int K, int per_layer, int obs_every,
                       int index_outputs, char* out, int out_len) {
    if (!out || out_len < 2) return fail(FG_ERR_BAD_ARG, "fg_describe_launch: out buffer required%s");
    int rc = check_params(params);
    if (rc) return rc;
    if (B <= 0 || K < 0) return fail(FG_ERR_BAD_ARG, "fg_describe_launch: B > 0 and K >= 0 required%s");
    out[0] = 0;
    const DescribeScope describing(out, out_len);
    if (scenario) {
        if ((rc = scenario_check(params, scenario, B, N, 1, K < 1 ? 1 : K, obs_every < 1 ? 1 : obs_every))) return rc;
        ScnArgs a; memset(&a, 0, sizeof(a));
        scn_args(&a, params, scenario, B, N, 1, K < 1 ? 1 : K, obs_every);
        return scenario_dispatch(a, nullptr);
    }
    if ((rc = hd_n_check(N))) return rc;
    Args a;
    if ((rc = hd_args(&a, params, B, N, K < 1 ? 1 : K, obs_every, 1, 1))) return rc;
    float* const f = reinterpret_cast<float*>((uintptr_t)4096);
    int32_t* const i32 = reinterpret_cast<int32_t*>((uintptr_t)4096);
    hd_buffers(&a, f, f, f, f, f, f, i32, f, f, f, reinterpret_cast<uint8_t*>((uintptr_t)4096));
    a.act = f;
    if (index_outputs) { a.near_lm = i32; a.near_ag = i32; a.hd_idx = i32; }
    if (per_layer > 0) {
        if (!policy_levels_for(N, per_layer, &a.pl)) return fail(FG_ERR_UNSUPPORTED_N, "N must be per_layer^L with 2 <= per_layer <= 8%s");
        a.act_out = f;
        return rollout_hd_policy_dispatch(a, per_layer, nullptr);
    }
    return K == 0 ? step_hd_dispatch(a, nullptr) : rollout_hd_dispatch(a, nullptr);   // fg_step_hd : fg_rollout_hd with K steps
}

int fg_rollout_hd_obs16(const FgParams* params, int obs_format, int B, int N, int K,
                        float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                        const float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                        void* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq,
                        int obs_every, void* stream) {
    const HdRollout r = {pos_x, pos_y, vel_x, vel_y, const_cast<float*>(act_seq), ideal_shape, ideal_vel, step,
                         static_cast<float*>(obs_seq), reward_seq, indiv_seq, done_seq};
    return obs16_rollout("fg_rollout_hd_obs16", params, obs_format, B, N, K, 0, r, obs_every, stream);
}

int fg_rollout_hd_policy_obs16(const FgParams* params, int obs_format, int B, int N, int K, int per_layer,
                               float* pos_x, float* pos_y, float* vel_x, float* vel_y,
                               float* act_seq, float* ideal_shape, float* ideal_vel, int32_t* step,
                               void* obs_seq, float* reward_seq, float* indiv_seq, uint8_t* done_seq,
                               int obs_every, void* stream) {
    if (per_layer == 0) return fail(FG_ERR_UNSUPPORTED_N, "%s: the closed loop needs per_layer = 3", "fg_rollout_hd_policy_obs16");
    const HdRollout r = {pos_x, pos_y, vel_x, vel_y, act_seq, ideal_shape, ideal_vel, step,
                         static_cast<float*>(obs_seq), reward_seq, indiv_seq, done_seq};
    return obs16_rollout("fg_rollout_hd_policy_obs16", params, obs_format, B, N, K, per_layer, r, obs_every, stream);
}

// The dry run of fg_rollout_hd_obs16 (per_layer 0) / fg_rollout_hd_policy_obs16 (per_layer 3): their checks before the buffers,
// then their dispatch.  Touches no device.
int fg_describe_obs16_launch(const FgParams* params, int obs_format, int B, int N, int K, int per_layer, int obs_every,
                             char* out, int out_len) {
    if (!out || out_len < 2) return fail(FG_ERR_BAD_ARG, "fg_describe_obs16_launch: out buffer required%s");
    out[0] = 0;
    FgPolicyLevels pl;
    int rc = obs16_check("fg_describe_obs16_launch", params, obs_format, B, N, K, per_layer, &pl);
    if (rc) return rc;
    if (B <= 0) return fail(FG_ERR_BAD_ARG, "fg_describe_obs16_launch: B > 0 required%s");
    Args a;
    if ((rc = hd_args(&a, params, B, N, K, obs_every, 1, 1))) return rc;
    const DescribeScope describing(out, out_len);
    return obs16_dispatch(a, obs_format, per_layer, nullptr);
}

int fg_rollout_hd_returns(const FgParams* params, int B, int N, int K, int C, float gamma,
                          const float* pos_x, const float* pos_y, const float* vel_x, const float* vel_y,
                          const float* ideal_shape, const float* ideal_vel, const int32_t* step,
                          const float* act, float* ret, float* indiv_ret, int32_t* steps, void* stream) {
    const int rc = returns_check(params, B, N, K, C, gamma);
    if (rc) return rc;
    if (B == 0) return FG_OK;                         // an empty batch: nothing to do
    ReturnsArgs a;
    if (const int rb = returns_args("fg_rollout_hd_returns", "%s: act/ideal_shape/ideal_vel must be 8-byte, the other buffers 4-byte aligned",
                                    &a, params, B, K, C, gamma, pos_x, pos_y, vel_x, vel_y, ideal_shape, ideal_vel, step, act, ret,
                                    indiv_ret, steps))
        return rb;
    a.act = act;
    const DeviceGuard device_guard(stream, pos_x);
    return returns_dispatch(a, N, (hipStream_t)stream);
}

int fg_describe_returns_launch(const FgParams* params, int B, int N, int K, int C, char* text, int cap) {
    if (!text || cap < 2) return fail(FG_ERR_BAD_ARG, "fg_describe_returns_launch: out buffer required%s");
    text[0] = 0;
    const int rc = returns_check(params, B, N, K, C, 1.0f);
    if (rc || B == 0) return rc;                      // an empty batch: FG_OK and no launch to name
    ReturnsArgs a;
    memset(&a, 0, sizeof(a));
    a.p = *params; a.B = B; a.K = K; a.C = C; a.gamma = 1.0f;
    const DescribeScope describing(text, cap);
    return returns_dispatch(a, N, nullptr);
}

// ---- a sampling planner's candidates (fg_planner_kernels.hpp) ----
int fg_rollout_hd_returns_sampled(const FgParams* params, int B, int N, int K, int C, float gamma, uint64_t noise_offset,
                                  float sigma, float clip,
                                  const float* pos_x, const float* pos_y, const float* vel_x, const float* vel_y,
                                  const float* ideal_shape, const float* ideal_vel, const int32_t* step,
                                  const float* mean, float* ret, float* indiv_ret, int32_t* steps, void* stream) {
    const char* const who = "fg_rollout_hd_returns_sampled";
    int rc = returns_check(params, B, N, K, C, gamma, who);
    if (rc || (rc = plan_check(who, B, N, K, C, sigma))) return rc;
    if (B == 0) return FG_OK;                         // an empty batch: nothing to do
    ReturnsSampledArgs a;
    if ((rc = returns_args(who, "%s: mean/ideal_shape/ideal_vel must be 8-byte, the other buffers 4-byte aligned", &a.r, params, B, K,
                           C, gamma, pos_x, pos_y, vel_x, vel_y, ideal_shape, ideal_vel, step, mean, ret, indiv_ret, steps)))
        return rc;
    a.mean = mean;
    a.d = plan_draw_of(params, noise_offset, sigma, clip);
    const DeviceGuard device_guard(stream, pos_x);
    return returns_dispatch(a, N, (hipStream_t)stream);
}

int fg_describe_returns_sampled_launch(const FgParams* params, int B, int N, int K, int C, char* text, int cap) {
    return describe_sampled<ReturnsSampledArgs>("fg_describe_returns_sampled_launch", "fg_rollout_hd_returns_sampled", params, B, N, K,
                                                C, text, cap);
}

// ---- ... with a sigma per step, env, agent and component: the cross-entropy method ----
int fg_rollout_hd_returns_sampled_std(const FgParams* params, int B, int N, int K, int C, float gamma, uint64_t noise_offset,
                                      float clip,
                                      const float* pos_x, const float* pos_y, const float* vel_x, const float* vel_y,
                                      const float* ideal_shape, const float* ideal_vel, const int32_t* step,
                                      const float* mean, const float* sd, float* ret, float* indiv_ret, int32_t* steps,
                                      void* stream) {
    const char* const who = "fg_rollout_hd_returns_sampled_std";
    const char* const aligned = "%s: mean/std/ideal_shape/ideal_vel must be 8-byte, the other buffers 4-byte aligned";
    int rc = returns_check(params, B, N, K, C, gamma, who);
    if (rc || (rc = plan_check(who, B, N, K, C, 0.0f))) return rc;
    if (B == 0) return FG_OK;                         // an empty batch: nothing to do
    ReturnsSampledStdArgs a;
    if ((rc = returns_args(who, aligned, &a.r, params, B, K, C, gamma, pos_x, pos_y, vel_x, vel_y, ideal_shape, ideal_vel, step, mean,
                           ret, indiv_ret, steps)))
        return rc;
    if (!sd) return null_pointer(who);
    if ((uintptr_t)sd & 7u) return fail(FG_ERR_ALIGNMENT, aligned, who);
    a.mean = mean;
    a.sd = sd;
    a.d = plan_draw_of(params, noise_offset, 0.0f, clip);
    const DeviceGuard device_guard(stream, pos_x);
    return returns_dispatch(a, N, (hipStream_t)stream);
}

int fg_describe_returns_sampled_std_launch(const FgParams* params, int B, int N, int K, int C, char* text, int cap) {
    return describe_sampled<ReturnsSampledStdArgs>("fg_describe_returns_sampled_std_launch", "fg_rollout_hd_returns_sampled_std",
                                                   params, B, N, K, C, text, cap);
}

int fg_plan_candidates_std(const FgParams* params, int B, int N, int K, int C, uint64_t noise_offset, float clip,
                           const float* mean, const float* sd, float* act_out, void* stream) {
    const char* const who = "fg_plan_candidates_std";
    int rc = check_params(params);
    if (rc || (rc = plan_check(who, B, N, K, C, 0.0f))) return rc;
    if (B == 0) return FG_OK;
    if (!sd || !act_out) return null_pointer(who);
    if (((uintptr_t)mean | (uintptr_t)sd | (uintptr_t)act_out) & 7u)
        return fail(FG_ERR_ALIGNMENT, "%s: mean, std and act_out must be 8-byte aligned", who);
    const unsigned grid = plan_grid((long long)C * K * B * N);
    if (!grid) return fail(FG_ERR_BAD_ARG, "%s: C * K * B * N must be below 2^39", who);
    const DeviceGuard device_guard(stream, act_out);
    return launch<&plan_candidates_std_kernel>(grid, 256, 0, (hipStream_t)stream, "plan candidates launch failed: %s",
                                               plan_draw_of(params, noise_offset, 0.0f, clip), B, N, K, C,
                                               reinterpret_cast<const float2*>(mean), reinterpret_cast<const float2*>(sd),
                                               reinterpret_cast<float2*>(act_out));
}

int fg_plan_cem_update(const FgParams* params, int B, int N, int K, int C, int E, uint64_t noise_offset, float clip, float alpha,
                       float sigma_min, const float* ret, const float* mean_in, const float* std_in, float* mean_out,
                       float* std_out, float* act_out, int32_t* elite_idx, int shift, void* stream) {
    const char* const who = "fg_plan_cem_update";
    int rc = check_params(params);
    if (rc || (rc = plan_check(who, B, N, K, C, 0.0f))) return rc;
    if (E < 1 || E > C) return fail(FG_ERR_BAD_ARG, "%s: 1 <= E <= C required", who);
    if (!(alpha > 0.0f && alpha <= 1.0f)) return fail(FG_ERR_BAD_ARG, "%s: alpha must be a finite number in (0, 1]", who);
    if (!(sigma_min >= 0.0f) || !std::isfinite(sigma_min)) return fail(FG_ERR_BAD_ARG, "%s: sigma_min must be a finite number >= 0", who);
    if (shift != 0 && shift != 1) return fail(FG_ERR_BAD_ARG, "%s: shift must be 0 or 1", who);
    if (B == 0) return FG_OK;
    if (!ret || !mean_in || !std_in || !mean_out || !std_out) return null_pointer(who);
    if ((((uintptr_t)mean_in | (uintptr_t)std_in | (uintptr_t)mean_out | (uintptr_t)std_out | (uintptr_t)act_out) & 7u) ||
        (((uintptr_t)ret | (uintptr_t)elite_idx) & 3u))
        return fail(FG_ERR_ALIGNMENT, "%s: mean_in, std_in, mean_out, std_out and act_out must be 8-byte, ret and elite_idx 4-byte aligned", who);
    const long long rows = (long long)B * N;
    const long long grid = (rows + FG_CEM_ROWS - 1) / FG_CEM_ROWS;
    if (grid > 0x7fffffffLL) return fail(FG_ERR_BAD_ARG, "%s: B * N must be below 2^33", who);
    // a row's wave writes row k - shift of the outputs while other waves still read the inputs: every output apart from
    // every input and from every other output (NULL: absent)
    const uintptr_t plan_bytes = (uintptr_t)K * B * N * sizeof(float2);
    struct Span { const void* p; uintptr_t n; };
    const Span in[3] = {{ret, (uintptr_t)C * B * N * sizeof(float)}, {mean_in, plan_bytes}, {std_in, plan_bytes}};
    const Span out[4] = {{mean_out, plan_bytes}, {std_out, plan_bytes}, {act_out, (uintptr_t)B * N * sizeof(float2)},
                         {elite_idx, (uintptr_t)E * B * N * sizeof(int32_t)}};
    const auto meet = [](const Span& x, const Span& y) {
        return x.p && y.p && (uintptr_t)x.p < (uintptr_t)y.p + y.n && (uintptr_t)y.p < (uintptr_t)x.p + x.n;
    };
    for (int o = 0; o < 4; ++o) {
        bool bad = false;
        for (int j = 0; j < 3; ++j) bad = bad || meet(out[o], in[j]);
        for (int j = 0; j < o; ++j) bad = bad || meet(out[o], out[j]);
        if (bad)
            return fail(FG_ERR_BAD_ARG, "%s: mean_out, std_out, act_out and elite_idx must not overlap ret, mean_in, std_in or each other", who);
    }
    CemArgs a;
    a.d = plan_draw_of(params, noise_offset, 0.0f, clip);
    a.B = B; a.N = N; a.K = K; a.C = C; a.E = E; a.shift = shift; a.alpha = alpha; a.sigma_min = sigma_min;
    a.ret = ret;
    a.mean_in = reinterpret_cast<const float2*>(mean_in); a.std_in = reinterpret_cast<const float2*>(std_in);
    a.mean_out = reinterpret_cast<float2*>(mean_out); a.std_out = reinterpret_cast<float2*>(std_out);
    a.act_out = reinterpret_cast<float2*>(act_out); a.elite_idx = elite_idx;
    const DeviceGuard device_guard(stream, mean_in);
    const hipStream_t st = (hipStream_t)stream;
    const char* const failed = "plan cem update launch failed: %s";
    constexpr int T = 64 * FG_CEM_ROWS;
    // the keys of a row in 1, 8 or 64 registers per lane; beyond FG_CEM_REG_C candidates they are re-read
    if (C <= 64) return launch<&plan_cem_update_kernel<1>>((unsigned)grid, T, 0, st, failed, a);
    if (C <= 512) return launch<&plan_cem_update_kernel<8>>((unsigned)grid, T, 0, st, failed, a);
    if (C <= FG_CEM_REG_C) return launch<&plan_cem_update_kernel<FG_CEM_REG_C / 64>>((unsigned)grid, T, 0, st, failed, a);
    return launch<&plan_cem_update_kernel<0>>((unsigned)grid, T, 0, st, failed, a);
}

int fg_plan_candidates(const FgParams* params, int B, int N, int K, int C, uint64_t noise_offset, float sigma, float clip,
                       const float* mean, float* act_out, void* stream) {
    const char* const who = "fg_plan_candidates";
    int rc = check_params(params);
    if (rc || (rc = plan_check(who, B, N, K, C, sigma))) return rc;
    if (B == 0) return FG_OK;
    if (!act_out) return null_pointer(who);
    if (((uintptr_t)mean | (uintptr_t)act_out) & 7u) return fail(FG_ERR_ALIGNMENT, "%s: mean and act_out must be 8-byte aligned", who);
    const unsigned grid = plan_grid((long long)C * K * B * N);
    if (!grid) return fail(FG_ERR_BAD_ARG, "%s: C * K * B * N must be below 2^39", who);
    const DeviceGuard device_guard(stream, act_out);
    return launch<&plan_candidates_kernel>(grid, 256, 0, (hipStream_t)stream, "plan candidates launch failed: %s",
                                           plan_draw_of(params, noise_offset, sigma, clip), B, N, K, C,
                                           reinterpret_cast<const float2*>(mean), reinterpret_cast<float2*>(act_out));
}

int fg_plan_mppi_update(const FgParams* params, int B, int N, int K, int C, uint64_t noise_offset, float sigma, float clip,
                        float lambda, const float* ret, const float* mean_in, float* mean_out, float* act_out, int shift,
                        void* stream) {
    const char* const who = "fg_plan_mppi_update";
    int rc = check_params(params);
    if (rc || (rc = plan_check(who, B, N, K, C, sigma))) return rc;
    if (!(lambda > 0.0f) || !std::isfinite(lambda)) return fail(FG_ERR_BAD_ARG, "%s: lambda must be a finite number > 0", who);
    if (shift != 0 && shift != 1) return fail(FG_ERR_BAD_ARG, "%s: shift must be 0 or 1", who);
    if (B == 0) return FG_OK;
    if (!ret || !mean_in || !mean_out) return null_pointer(who);
    if ((((uintptr_t)mean_in | (uintptr_t)mean_out | (uintptr_t)act_out) & 7u) || ((uintptr_t)ret & 3u))
        return fail(FG_ERR_ALIGNMENT, "%s: mean_in, mean_out and act_out must be 8-byte, ret 4-byte aligned", who);
    const unsigned grid = plan_grid((long long)K * B * N);
    if (!grid) return fail(FG_ERR_BAD_ARG, "%s: K * B * N must be below 2^39", who);
    // thread (k, b, i) writes row k - shift: another thread's input
    const uintptr_t bytes = (uintptr_t)K * B * N * sizeof(float2), in = (uintptr_t)mean_in, out = (uintptr_t)mean_out;
    if (in < out + bytes && out < in + bytes) return fail(FG_ERR_BAD_ARG, "%s: mean_out must not overlap mean_in", who);
    // ... and the outputs are written while other threads still read `ret` and `mean_in`: each output apart from each input
    // and from the other output
    const uintptr_t ret_bytes = (uintptr_t)C * B * N * sizeof(float), rt = (uintptr_t)ret;
    const uintptr_t act_bytes = (uintptr_t)B * N * sizeof(float2), ao = (uintptr_t)act_out;
    const auto meet = [](uintptr_t x, uintptr_t nx, uintptr_t y, uintptr_t ny) { return x < y + ny && y < x + nx; };
    if (meet(out, bytes, rt, ret_bytes) ||
        (act_out && (meet(ao, act_bytes, in, bytes) || meet(ao, act_bytes, rt, ret_bytes) || meet(ao, act_bytes, out, bytes))))
        return fail(FG_ERR_BAD_ARG, "%s: mean_out and act_out must not overlap ret, mean_in or each other", who);
    const DeviceGuard device_guard(stream, mean_in);
    return launch<&plan_mppi_update_kernel>(grid, 256, 0, (hipStream_t)stream, "plan update launch failed: %s",
                                            plan_draw_of(params, noise_offset, sigma, clip), B, N, K, C, lambda, ret,
                                            reinterpret_cast<const float2*>(mean_in), reinterpret_cast<float2*>(mean_out),
                                            reinterpret_cast<float2*>(act_out), shift);
}

}  // extern "C"
