// r06_zero_skip/holes.hip - pure-store microbenchmark (no library code): does the 27-agent observation stream get faster when
// the stores into the rows' zero block (units [N, 2N-1) of every 3N-unit row: 208 of 648 bytes) are left out?
//   hipcc --offload-arch=gfx950 -O3 -o holes profiles/r06_zero_skip/holes.hip && ./holes
// Geometry of the headline (fg_rollout_hd, 27 agents x 4096 envs x 20 steps): 256 workgroups x 8 storing waves, workgroup g
// owns the 16 consecutive env blocks (17 496 B each, one span of 2 187 whole 128-byte lines) of every slab, wave w the envs
// w and w + 8 cut at the 128-byte lines (line ownership of write_obs_tiled), 1 KiB per store instruction (16 B per lane),
// one s_sleep(1) behind every instruction as in the writer's stream(); 20 slabs into a 1.43 GB buffer (ordinary hipMalloc).
// A hole must not make the remaining requests partial (r02_store/env_order.txt: leaving out a 40-byte pad cost 8 %), so the
// aligned arms leave out only whole address-aligned groups that lie wholly inside ONE row's zero block:
//   full      every byte written                                              (the writer today)
//   skip64    whole 64-byte groups of the zero block left out                 (2.375 groups = 152 B of 648 per row on average)
//   skip128   whole 128-byte lines of the zero block left out                 (0.69 lines = 88 B per row on average)
//   exact     control: exactly the 208 bytes left out, 8-byte stores at the block's odd edges (partial requests)
// The arms run alternately, PASSES times; an arm is "clearly faster" iff every pass of it beats every pass of "full".
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

constexpr int N = 27, ROWB = 3 * N * 8, ENVB = ROWB * N;             // 648 B per row, 17 496 B per env
constexpr int Z0 = N * 8, Z1 = (2 * N - 1) * 8;                      // the zero block of a row: bytes [216, 424)
constexpr int K = 20, B = 4096, G = 256, E = 16, NW = 8;
constexpr unsigned SPAN = (unsigned)E * ENVB;                          // 279 936 B = 2 187 lines per workgroup and slab

__device__ __forceinline__ bool in_zero(unsigned o) {                 // o: byte offset inside an env block
    const unsigned off = o % ROWB;
    return off >= Z0 && off < Z1;
}
// a: byte offset of the lane's 16 bytes inside the slab.  GB-aligned group around it wholly inside one row's zero block?
template <unsigned GB> __device__ __forceinline__ bool group_in_zero(unsigned a) {
    const unsigned g0 = a & ~(GB - 1), es = (a / ENVB) * ENVB;
    if (g0 < es || g0 + GB > es + ENVB) return false;                  // reaches into a neighbouring env
    const unsigned off = (g0 - es) % ROWB;
    return off >= Z0 && off + GB <= Z1;
}

template <int ARM> __global__ __launch_bounds__(NW * 64) void k_holes(char* out) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const f32x4 v = {1.f, 2.f, 3.f, 4.f};
    for (int k = 0; k < K; ++k) {
        char* slab = out + (size_t)k * B * ENVB;                       // 128-byte aligned: B * ENVB = 559 872 lines
        const unsigned span0 = blockIdx.x * SPAN;
        for (int e = w; e < E; e += NW) {
            const unsigned s = span0 + (((unsigned)e * ENVB + 127u) & ~127u);
            const unsigned end = span0 + (e + 1 == E ? SPAN : (((unsigned)(e + 1) * ENVB + 127u) & ~127u));
            for (unsigned a0 = s; a0 < end; a0 += 1024u) {             // wave-uniform trip count
                const unsigned a = a0 + 16u * lane;
                if (a < end) {
                    if (ARM == 0) {
                        *reinterpret_cast<f32x4*>(slab + a) = v;
                    } else if (ARM == 1) {
                        if (!group_in_zero<64>(a)) *reinterpret_cast<f32x4*>(slab + a) = v;
                    } else if (ARM == 2) {
                        if (!group_in_zero<128>(a)) *reinterpret_cast<f32x4*>(slab + a) = v;
                    } else {
                        const unsigned o = a % ENVB;                   // a and a + 8 lie in the same env: ENVB is a multiple of 8, a of 16
                        const bool z0 = in_zero(o), z1 = in_zero(o + 8 < ENVB ? o + 8 : 0);
                        if (!z0 && !z1) *reinterpret_cast<f32x4*>(slab + a) = v;
                        else if (!z0) *reinterpret_cast<f32x2*>(slab + a) = f32x2{1.f, 2.f};
                        else if (!z1) *reinterpret_cast<f32x2*>(slab + a + 8) = f32x2{3.f, 4.f};
                    }
                }
                asm volatile("" ::: "memory");
                __builtin_amdgcn_s_sleep(1);
            }
        }
    }
}

template <int ARM> float run(char* buf, hipEvent_t e0, hipEvent_t e1, int reps) {
    for (int i = 0; i < 3; ++i) hipLaunchKernelGGL(k_holes<ARM>, dim3(G), dim3(NW * 64), 0, 0, buf);
    CHECK(hipEventRecord(e0));
    for (int i = 0; i < reps; ++i) hipLaunchKernelGGL(k_holes<ARM>, dim3(G), dim3(NW * 64), 0, 0, buf);
    CHECK(hipEventRecord(e1));
    CHECK(hipEventSynchronize(e1));
    float ms; CHECK(hipEventElapsedTime(&ms, e0, e1));
    return ms / reps * 1e3f;
}

int main() {
    const size_t bytes = (size_t)K * B * ENVB;
    char* buf;
    CHECK(hipMalloc(&buf, bytes + 4096));
    CHECK(hipMemset(buf, 0, bytes + 4096));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    // bytes each arm stores, counted on the host with the device's own rule
    double stored[4] = {0, 0, 0, 0};
    for (unsigned a = 0; a < (unsigned)B * ENVB; a += 16) {
        auto giz = [&](unsigned GB) {
            const unsigned g0 = a & ~(GB - 1), es = (a / ENVB) * ENVB;
            if (g0 < es || g0 + GB > es + ENVB) return false;
            const unsigned off = (g0 - es) % ROWB;
            return off >= (unsigned)Z0 && off + GB <= (unsigned)Z1;
        };
        auto iz = [&](unsigned x) { const unsigned off = (x % ENVB) % ROWB; return off >= (unsigned)Z0 && off < (unsigned)Z1; };
        stored[0] += 16;
        stored[1] += giz(64) ? 0 : 16;
        stored[2] += giz(128) ? 0 : 16;
        stored[3] += (iz(a) ? 0 : 8) + (iz(a + 8) ? 0 : 8);
    }
    const char* names[4] = {"full", "skip64", "skip128", "exact"};
    for (int i = 0; i < 4; ++i) printf("%-8s stores %.1f %% of the bytes\n", names[i], 100.0 * stored[i] / stored[0]);
    const int PASSES = 6, REP = 20;
    float lo[4] = {1e30f, 1e30f, 1e30f, 1e30f}, hi[4] = {0, 0, 0, 0};
    for (int pass = 0; pass < PASSES; ++pass)
        for (int arm = 0; arm < 4; ++arm) {
            const float us = arm == 0 ? run<0>(buf, e0, e1, REP) : arm == 1 ? run<1>(buf, e0, e1, REP)
                           : arm == 2 ? run<2>(buf, e0, e1, REP) : run<3>(buf, e0, e1, REP);
            lo[arm] = us < lo[arm] ? us : lo[arm]; hi[arm] = us > hi[arm] ? us : hi[arm];
            printf("pass %d  %-8s  %.1f us/launch  %.2f us/slab  %.2f TB/s (bytes a consumer sees)\n", pass, names[arm], us, us / K,
                   (double)bytes / (us * 1e-6) / 1e12);
        }
    for (int arm = 0; arm < 4; ++arm)
        printf("%-8s  %.1f - %.1f us/launch%s\n", names[arm], lo[arm], hi[arm],
               arm == 0 ? "" : hi[arm] < lo[0] ? "  every pass faster than every pass of full" : "  NOT clearly faster than full");
    CHECK(hipFree(buf));
    return 0;
}
