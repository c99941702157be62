// fg_scn_kernel.hpp - The run-time-count kernel of the landmark scenarios (fg::scn_kernel), its argument block, its LDS size
// and the counter-RNG draws of its fused auto-reset.  The arithmetic type is a parameter (`real` of fg_common.hpp), as
// step_kernel's is: the product library builds it in fp32 (included by fg_aux_kernels.hpp), formation_hip_f64.hip builds the
// SAME source with real = double (fg64_rollout_scenario, tests only), where it free-runs on the reference's fixtures.
#ifndef FG_SCN_KERNEL_HPP_
#define FG_SCN_KERNEL_HPP_

#include "fg_common.hpp"

namespace fg {

// ---------------------------------------------------------------------------
// Landmark scenarios (N + M <= 1024 movable entities): basic_formation_env (BASELINE config 1),
// formation_hd_partial_env, formation_hd_partial_range_env, formation_hd_obs_env.
// One lane per movable entity (N agents, then M obstacles), one env per aligned group of G
// lanes of a wave (N + M <= 64) or per workgroup of G threads (beyond).  Reference lines under formation_gym/envs/:
//   basic     observation basic_formation_env.py:29-41, reward :43-52 (self "collision" included)
//   partial   observation formation_hd_partial_env.py:38-57 (ring neighbours), reward :59-72
//   range     observation formation_hd_partial_range_env.py:38-52 (clipped), reward as partial
//   obstacle  observation formation_hd_obs_env.py:44-58, reward :60-99 incl. the obstacle
//             velocity override (:84-89); obstacles are movable colliders of World.step
// ---------------------------------------------------------------------------
// The scenario constants as the kernel reads them: the C ABI's FgScenario (fp32 lengths), or the same fields with the six
// lengths in double for the parity build (0.15f is not the reference's 0.15, 0.7f not its 0.7)
#if FG_F64
struct KScenario {
    int32_t kind, num_landmarks, num_obstacles, num_obs;
    double obs_range, obstacle_size, obstacle_vx, obstacle_vy, obstacle_floor, penalty;
    int32_t variant, reserved;
};
#else
typedef FgScenario KScenario;
#endif

struct ScnArgs {
    KParams p;
    KScenario sc;
    int B, N, do_phys;
    real* px; real* py; real* vx; real* vy;
    const real* act; real* lm; real* opos; real* ovel; int32_t* step;
    real* obs; real* rew; real* indiv; uint8_t* done; int32_t* near_ag;
    int stage;     // compose the workgroup's observation rows in LDS and stream them out as ONE contiguous span
    int K;         // steps per launch (fg_rollout_scenario; 1 otherwise): act / reward / indiv / done / near_ag [K][B]...,
    int obs_every; // obs [K / obs_every][B][N][D]
    real coll_scale;      // per-agent tables (FgParams.agent_props): penalty distance of a pair = coll_scale * (size_a + size_b)
    real inv_n, inv_l;    // 1 / N, 1 / L, correctly rounded on the host: the run-time-count kernel and the one-env-per-lane
                          // kernels (compile-time counts) must multiply by the very same values (cf. Args.inv_n)
};

// Geometry and dynamic LDS of one scn_kernel workgroup.  G lanes per env = pow2 >= N + M, at least 4; up to 64 entities a
// workgroup of 64 threads holds 64 / G envs, beyond that one env is the whole workgroup of G threads.  LDS, in real2 units:
// the 32 cross-wave partials of env_reduce (G > 64 only), per env the tables PRE[N + M] | POST[N + M] | LM[L], and - staged
// launches - the image of the workgroup's [E][N][D] observation block behind the last env's tables.
constexpr int FG_SCN_T = 64;      // threads per workgroup of the scenario kernel up to 64 entities per env
__host__ __device__ constexpr int scn_envs_per_group(int G) { return G <= 64 ? FG_SCN_T / G : 1; }
__host__ __device__ constexpr int scn_group_lanes(int entities) {     // scn_kernel's G: pow2 >= N + M, at least 4
    int g = 4;
    while (g < entities) g <<= 1;
    return g;
}
__host__ __device__ constexpr int scn_obs_dim(int kind, int n, int l, int m, int nbr) {
    return 2 + (kind == FG_SCN_BASIC ? 2 : 0) + 2 * l + 2 * m + 2 * nbr + 2 * (n - 1);
}
// obs_dim = scn_obs_dim(...) of a staged launch (its image: E x N rows), 0 of one that writes its rows straight to memory
__host__ __device__ constexpr long long scn_lds_bytes(int G, int N, int L, int M, int obs_dim) {
    const long long E = scn_envs_per_group(G);
    return (E * (2 * (N + M) + L) + (G > 64 ? 32 : 0)) * (long long)sizeof(real2) + E * N * obs_dim * (long long)sizeof(real);
}

// Scenario.reset_world of these scenarios from the device counter RNG (basic_formation_env.py:54-65,
// formation_hd_partial_env.py:88-99, formation_hd_partial_range_env.py:76-87, formation_hd_obs_env.py:101-114): agents and landmarks U(-1,1)^2, velocities zero,
// obstacle k from U([s_k, 2.0], [s_k+1, 2.5]) with s = linspace(-1.8, 1.8, M + 1), falling at the scenario's velocity.
// One Philox block per entity, counter (global env index, entity code, per-launch offset); entity code = agent index,
// 0x10000000 | landmark index, 0x20000000 | obstacle index (formation_hd_env's reset uses the agent indices and
// 0xFFFFFFFF the same way).  Distributional parity with the reference's MT19937 draws, as for formation_hd_env.
// The draws are fp32 whatever `real` is, converted where they are returned.
constexpr uint32_t SCN_LANDMARK_CODE = 0x10000000u, SCN_OBSTACLE_CODE = 0x20000000u;
__device__ __forceinline__ real2 scn_fresh_pm1(const KParams& P, int b, uint32_t code, uint64_t off) {
    uint32_t c[4] = {(uint32_t)(b + P.env_index_base), code, (uint32_t)off, (uint32_t)(off >> 32)};
    philox4x32(c, (uint32_t)P.seed, (uint32_t)(P.seed >> 32));
    return make_real2(u_pm1(c[0]), u_pm1(c[1]));
}
__device__ __forceinline__ real2 scn_fresh_obstacle(const KParams& P, int b, int k, int M, uint64_t off) {
    const real2 r = scn_fresh_pm1(P, b, SCN_OBSTACLE_CODE | (uint32_t)k, off);
    const float lo = -1.8f + 3.6f * (float)k / (float)M, hi = -1.8f + 3.6f * (float)(k + 1) / (float)M;
    return make_real2(lo + (hi - lo) * (0.5f * (float)r.x + 0.5f), 2.0f + 0.5f * (0.5f * (float)r.y + 0.5f));
}

template <int G, int T>
__global__ __launch_bounds__(T) void scn_kernel(const ScnArgs a) {
    constexpr int E = T / G;
    extern __shared__ __attribute__((aligned(16))) real2 smem[];
    const int N = a.N, L = a.sc.num_landmarks, M = a.sc.num_obstacles, NE = N + M;
    const int kind = a.sc.kind;
    const int tid = threadIdx.x;
    const int e = tid / G, i = tid % G;
    const int b = blockIdx.x * E + e;
    const bool live = b < a.B;
    const bool is_agent = live && i < N;
    const bool is_obst = live && i >= N && i < NE;
    constexpr int SCR = (G > 64) ? 32 : 0;            // G > 64 (one env per workgroup): cross-wave partials of env_reduce
    real* const scratch = reinterpret_cast<real*>(smem);
    real2* const tables = smem + SCR;
    real2* const PRE = tables + e * (2 * NE + L);
    real2* const POST = PRE + NE;
    real2* const LM = POST + NE;
    real2 p = make_real2(0.f, 0.f), v = p;
    const size_t sidx = (size_t)b * N + i;
    const size_t oidx = (size_t)b * M + (i - N);
    if (is_agent) {
        p = make_real2(a.px[sidx], a.py[sidx]);
        v = make_real2(a.vx[sidx], a.vy[sidx]);
    } else if (is_obst) {
        p = reinterpret_cast<const real2*>(a.opos)[oidx];
        v = reinterpret_cast<const real2*>(a.ovel)[oidx];
    }
    if (is_agent || is_obst) { PRE[i] = p; POST[i] = p; }
    for (int l = i; live && l < L; l += G) LM[l] = reinterpret_cast<const real2*>(a.lm)[(size_t)b * L + l];
    int t_step = (live && a.step) ? a.step[b] : 0;
    __syncthreads();
    // agents of different mass / size / accel / max_speed / u_noise (FgParams.agent_props; core.py:45-109): the lane's own row;
    // its partners' mass and size are read from the table in the pair loops (a cold path: no reference scenario has them).
    // The obstacles keep the scenario's size and Entity's default mass 1 (formation_hd_obs_env.py:36-42).
    // Column 6 of the table = the agent's flags (core.py:54-58), honoured as step_kernel's option path does: a pair needs both
    // to collide (:292-293); against an immovable partner the force is taken as it is, not scaled by the mass ratio (:319-321);
    // an immovable agent is not integrated (:266-267); a ghost passes through soft walls (:326-327); the penalties of an agent
    // that does not collide are not counted (`if agent.collide:` in every reward callback).  The obstacles are ordinary colliders.
    const bool het = a.p.agent_props != nullptr;
    const AgentProps me = agent_props_of(a.p, i, het && i < N);
    const int my_flags = (het && i < N) ? me.flags : 0;
    const real my_size = i < N ? (het ? me.size : 0.5f * a.p.dist_min) : 0.5f * (2.0f * a.sc.obstacle_size);
    const real my_mass = het ? (i < N ? me.mass : 1.0f) : a.p.mass;
    const int KS = a.K > 1 ? a.K : 1;
    real2 u_next = make_real2(0.f, 0.f);                // the action of step ks + 1 is fetched while step ks runs
    if (a.do_phys && is_agent) u_next = reinterpret_cast<const real2*>(a.act)[sidx];
    // K steps in one launch (fg_rollout_scenario): the state stays in registers / LDS, every step's reward, done and (every
    // obs_every-th) observation go to their slab - the same arithmetic as K single-step launches, bit for bit
    const uint64_t rbase = rng_base(a.p);               // read once: no load from the device counter inside the step loop
    for (int ks = 0; ks < KS; ++ks) {
    const uint64_t off = rbase + (uint64_t)ks;
    const size_t kb = (size_t)ks * a.B;                 // slab of step ks in the [K][B]... outputs
    const real2 u_now = u_next;
    if (a.do_phys && is_agent && ks + 1 < KS) u_next = reinterpret_cast<const real2*>(a.act)[(kb + a.B) * N + sidx];
    if (a.do_phys) {
        if (is_agent || is_obst) {
            // World.step: all pairs of movable colliders, contact distance size_i + size_j
            real fx = 0.f, fy = 0.f;
            const real k = a.p.contact_margin;
            // (the loops of this kernel run over a handful of entities with run-time counts: four LDS reads are issued
            // ahead of their use, index clamped, so that a wave waits once per four partners instead of once per partner;
            // the order of the sums is the ascending-j order of core.py:240-262 either way)
            for (int j0 = 0; j0 < NE; j0 += 4) {
                real2 qq[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) qq[t] = PRE[min(j0 + t, NE - 1)];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int j = j0 + t;
                    const real2 q = qq[t];
                    real size_j = 0.5f * (j < N ? a.p.dist_min : 2.0f * a.sc.obstacle_size);
                    int fj = 0;
                    if (het && j < N) {
                        size_j = a.p.agent_props[(size_t)j * FG_AGENT_PROPS + 1];
                        fj = (int)a.p.agent_props[(size_t)j * FG_AGENT_PROPS + 6];
                    }
                    const real dmin = my_size + size_j;
                    const real cut = dmin + (FG_F64 ? 40.0f : 18.0f) * k;   // force beyond: < 1e2 k e^-18 ~ 1.5e-9 (fp64 build: e^-40)
                    const real dx = p.x - q.x, dy = p.y - q.y;
                    const real d2 = dx * dx + dy * dy;
                    if (j < NE && j != i && d2 < cut * cut && !((fj | my_flags) & FG_AGENT_NO_COLLIDE)) {
                        const real d = hw_sqrt(d2);
                        const real x = (dmin - d) / k;
                        const real pen = k * (rmax(x, real(0)) + hw_log(1.0f + hw_exp(-rabs(x))));
                        real c = a.p.contact_force * pen * hw_rcp(d);
                        if (het && !(fj & FG_AGENT_IMMOVABLE))
                            c = ((j < N ? a.p.agent_props[(size_t)j * FG_AGENT_PROPS] : 1.0f) / my_mass) * c;   // core.py:314-317
                        fx += dx * c; fy += dy * c;
                    }
                }
            }
            if (is_agent) {
                const real2 u = u_now;
                const real2 fa = action_force(a.p, me, u, (uint32_t)(b + a.p.env_index_base), (uint32_t)i, off);
                fx += fa.x; fy += fa.y;
            }
            if (a.p.num_walls > 0) wall_forces(a.p, p, my_size, fx, fy, (my_flags & FG_AGENT_GHOST) != 0);
            if (!(my_flags & FG_AGENT_IMMOVABLE)) {
                v.x = v.x * (1.0f - a.p.damping) + (fx / my_mass) * a.p.dt;
                v.y = v.y * (1.0f - a.p.damping) + (fy / my_mass) * a.p.dt;
                if (is_agent) v = clamp_speed(me.max_speed, v);
                p.x += v.x * a.p.dt; p.y += v.y * a.p.dt;
            }
            POST[i] = p;
            if (is_agent) {
                a.px[sidx] = p.x; a.py[sidx] = p.y; a.vx[sidx] = v.x; a.vy[sidx] = v.y;
            } else {
                // the reward callback re-arms the obstacle velocity every step (:84-89)
                const bool falling = p.y > a.sc.obstacle_floor;
                v = make_real2(falling ? a.sc.obstacle_vx : 0.f, falling ? a.sc.obstacle_vy : 0.f);   // what the next step loads
                reinterpret_cast<real2*>(a.opos)[oidx] = p;
                reinterpret_cast<real2*>(a.ovel)[oidx] = v;
            }
        }
        t_step += 1;
        __syncthreads();
    }
    // ---- formation term ----
    real form = 0.f;       // basic: sum_l min_a |p_a - l| ; others: Hausdorff(centred agents, centred landmarks)
    if (kind == FG_SCN_BASIC) {
        real cover = 0.f;
        for (int l0 = 0; l0 < L; l0 += G) {
            const int l = l0 + i;
            if (live && l < L) {
                const real2 m = LM[l];
                real best = INFINITY; int barg = 0;
                for (int j0 = 0; j0 < N; j0 += 4) {
                    real2 qq[4];
#pragma unroll
                    for (int t = 0; t < 4; ++t) qq[t] = POST[min(j0 + t, N - 1)];
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const real dx = qq[t].x - m.x, dy = qq[t].y - m.y, d2 = dx * dx + dy * dy;
                        if (j0 + t < N && d2 < best) { best = d2; barg = j0 + t; }
                    }
                }
                cover += rsqrt_(best);
                if (a.near_ag) a.near_ag[(kb + b) * L + l] = barg;
            }
        }
        real red[1] = {cover};
        env_reduce<G, T, 1, R_SUM, R_SUM, R_SUM, R_SUM>(red, scratch);
        form = red[0];
    } else {
        real s4[4] = {is_agent ? p.x : 0.f, is_agent ? p.y : 0.f, 0.f, 0.f};
        for (int l = i; live && l < L; l += G) { s4[2] += LM[l].x; s4[3] += LM[l].y; }
        env_reduce<G, T, 4, R_SUM, R_SUM, R_SUM, R_SUM>(s4, scratch);
        const real mx = s4[0] * a.inv_n, my = s4[1] * a.inv_n;
        const real lx = s4[2] * a.inv_l, ly = s4[3] * a.inv_l;
        real rowmin = -INFINITY, colmax = -INFINITY;
        if (is_agent) {                                         // min over landmarks for my agent
            rowmin = INFINITY;
            for (int l0 = 0; l0 < L; l0 += 4) {
                real2 mm[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) mm[t] = LM[min(l0 + t, L - 1)];
#pragma unroll
                for (int t = 0; t < 4; ++t) {                  // a clamped repeat of the last landmark does not change a minimum
                    const real dx = (p.x - mx) - (mm[t].x - lx), dy = (p.y - my) - (mm[t].y - ly);
                    rowmin = rmin(rowmin, dx * dx + dy * dy);
                }
            }
        }
        for (int l = i; live && l < L; l += G) {                // min over agents for my landmark(s)
            real cm = INFINITY;
            const real2 ml = LM[l];
            for (int j0 = 0; j0 < N; j0 += 4) {
                real2 qq[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) qq[t] = POST[min(j0 + t, N - 1)];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const real dx = (qq[t].x - mx) - (ml.x - lx), dy = (qq[t].y - my) - (ml.y - ly);
                    cm = rmin(cm, dx * dx + dy * dy);
                }
            }
            colmax = rmax(colmax, cm);
        }
        real red[2] = {rowmin, colmax};
        env_reduce<G, T, 2, R_MAX, R_MAX, R_MAX, R_MAX>(red, scratch);
        form = rsqrt_(rmax(red[0], red[1]));
    }
    // ---- collision counts ----
    int cnt = 0;
    if (is_agent) {
        // (fp32: the squares of the thresholds rounded once from the double product; fp64 build: plain products)
        const real thr = a.p.collide_thresh, thr2 = (real)((double)thr * (double)thr);
        for (int j0 = 0; j0 < N; j0 += 4) {
            real2 qq[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) qq[t] = POST[min(j0 + t, N - 1)];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int j = j0 + t;
                const real dx = qq[t].x - p.x, dy = qq[t].y - p.y;
                real t2 = thr2;
                if (het && j < N) {                               // is_collision per pair: dist < size_a + size_b
                    const real tj = a.coll_scale * (my_size + a.p.agent_props[(size_t)j * FG_AGENT_PROPS + 1]);
                    t2 = tj * tj;
                }
                cnt += (j < N && (kind == FG_SCN_BASIC || j != i) && dx * dx + dy * dy < t2) ? 1 : 0;
            }
        }
        const real ot = (het ? my_size : 0.5f * a.p.dist_min) + a.sc.obstacle_size, ot2 = (real)((double)ot * (double)ot);
        for (int j = N; j < NE; ++j) {
            const real dx = POST[j].x - p.x, dy = POST[j].y - p.y;
            cnt += (dx * dx + dy * dy < ot2) ? 1 : 0;
        }
    }
    if (my_flags & FG_AGENT_NO_COLLIDE) cnt = 0;
    real cs[1] = {(real)cnt};
    env_reduce<G, T, 1, R_SUM, R_SUM, R_SUM, R_SUM>(cs, scratch);
    const bool is_done = t_step >= a.p.world_length;
    // ---- outputs ----
    const int nbr = (kind == FG_SCN_PARTIAL) ? a.sc.num_obs : (N - 1);
    const int D = 2 + (kind == FG_SCN_BASIC ? 2 : 0) + 2 * L + 2 * M + 2 * nbr + 2 * (N - 1);
    if (is_agent) {
        if (a.rew) a.rew[kb * N + sidx] = (real)(-(double)N * (double)form - (double)a.sc.penalty * (double)cs[0]);
        if (a.indiv) a.indiv[kb * N + sidx] = -form - a.sc.penalty * (real)cnt;
        if (a.done) a.done[kb * N + sidx] = is_done ? 1 : 0;
    }
    if (a.p.auto_reset && a.do_phys) {                  // uniform over the launch
        // the vec-env worker's rule (env_wrappers.py:14-18): an env whose episode is over restarts at once, and the
        // observation returned with the finished step's reward / done is the RESET observation
        __syncthreads();                                // every lane has finished reading POST / LM of the finished step
        if (live && is_done) {
            if (is_agent) {
                p = scn_fresh_pm1(a.p, b, (uint32_t)i, off); v = make_real2(0.f, 0.f);
                POST[i] = p;
                a.px[sidx] = p.x; a.py[sidx] = p.y; a.vx[sidx] = 0.f; a.vy[sidx] = 0.f;
            } else if (is_obst) {
                p = scn_fresh_obstacle(a.p, b, i - N, M, off);
                v = make_real2(a.sc.obstacle_vx, a.sc.obstacle_vy);
                POST[i] = p;
                reinterpret_cast<real2*>(a.opos)[oidx] = p;
                reinterpret_cast<real2*>(a.ovel)[oidx] = v;
            }
            for (int l = i; l < L; l += G) {
                const real2 m = scn_fresh_pm1(a.p, b, SCN_LANDMARK_CODE | (uint32_t)l, off);
                LM[l] = m;
                reinterpret_cast<real2*>(a.lm)[(size_t)b * L + l] = m;
            }
            t_step = 0;
        }
        __syncthreads();
    }
    const bool want_obs = a.obs_every <= 1 || (ks + 1) % a.obs_every == 0;
    const size_t ob = (size_t)(a.obs_every > 1 ? ks / a.obs_every : ks) * a.B;   // slab of this step's observation
    if (is_agent && want_obs) {
        // every lane composes its own row: straight to global memory (rows D floats apart: one 8-byte piece per lane
        // and instruction), or into the workgroup's LDS image of its [E][N][D] block, which all lanes then copy out
        // with consecutive 8-byte stores (a.stage; 16 x 65536 obstacle envs: 203 -> see profiles/r02_aux_kernels.md)
        real2* const stage0 = tables + E * (2 * NE + L);                               // behind the last env's tables
        real2* o = a.stage ? stage0 + (size_t)(e * N + i) * (D / 2) : reinterpret_cast<real2*>(a.obs + (ob * N + sidx) * D);
        int w = 0;
        o[w++] = v;
        if (kind == FG_SCN_BASIC) o[w++] = p;
        // a segment of `count` units, unit t = get(t): four sources are read before the four stores (the staged row lives in
        // LDS like the tables, so a read behind a store would have to wait for it)
        auto emit = [&](int count, auto&& get) {
            for (int t0 = 0; t0 < count; t0 += 4) {
                real2 r[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) r[t] = get(min(t0 + t, count - 1));
#pragma unroll
                for (int t = 0; t < 4; ++t) if (t0 + t < count) o[w + t] = r[t];
                w += min(4, count - t0);
            }
        };
        const bool basic = kind == FG_SCN_BASIC;
        emit(L, [&](int l) { const real2 m = LM[l]; return basic ? make_real2(m.x - p.x, m.y - p.y) : m; });
        emit(M, [&](int t) { const real2 q = POST[N + t]; return make_real2(q.x - p.x, q.y - p.y); });
        if (kind == FG_SCN_PARTIAL) {
            emit(nbr, [&](int kk) {
                int j = i + 1 + kk;                            // (i + 1 + kk) mod N
                while (j >= N) j -= N;
                const real2 q = POST[j];
                return make_real2(q.x - p.x, q.y - p.y);
            });
        } else {
            const real r = (kind == FG_SCN_RANGE) ? a.sc.obs_range : INFINITY;
            emit(N - 1, [&](int t) {
                const real2 q = POST[t < i ? t : t + 1];      // the t-th OTHER agent, index order
                return make_real2(rmin(rmax(q.x - p.x, -r), r), rmin(rmax(q.y - p.y, -r), r));
            });
        }
        for (int j = 0; j < N - 1; ++j) o[w++] = make_real2(0.f, 0.f);
    }
    if (a.stage && want_obs) {                          // want_obs is uniform over the launch
        __syncthreads();
        const real2* const img = tables + E * (2 * NE + L);
        const int b0 = blockIdx.x * E;
        const int El = min(E, a.B - b0);
        const int units = El * N * (D / 2);
        real2* const out = reinterpret_cast<real2*>(a.obs + (ob + (size_t)b0) * N * D);
        for (int q0 = tid; q0 < units; q0 += 4 * T) {
            real2 r[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) r[t] = img[min(q0 + t * T, units - 1)];
#pragma unroll
            for (int t = 0; t < 4; ++t) if (q0 + t * T < units) out[q0 + t * T] = r[t];
        }
    }
    if (ks + 1 < KS) {                                  // the next step starts from this one's end state
        __syncthreads();                                // POST read by everyone, the staged image copied out
        if (is_agent || is_obst) PRE[i] = p;
        __syncthreads();
    }
    }   // steps
    if (a.do_phys && a.step && live && i == 0) a.step[b] = t_step;
}

}  // namespace fg

#endif  // FG_SCN_KERNEL_HPP_
