// fg_actor_kernel_pair.inc - the two kernels of one formation_hd_env actor family (fg_actor_rollout_kernel.hpp): the
// deterministic actor and its Gaussian twin, which takes (log_std, logp) after the family's operands.  The family block
// that includes this file defines
//     FG_ACTOR_DET, FG_ACTOR_SMP   the two kernel names
//     FG_ACTOR_FLAGS               `PER_AGENT = .., LNORM = .., GRU = .., INBN = ..` (the declarators after SAMPLE)
//     FG_ACTOR_OPERANDS            the kernel parameters after `a`
//     FG_ACTOR_ABSENT              the FG_ACTOR_NO_* constants of the operands the family does not take
//     FG_ACTOR_OUK (optional)      the name of the family's third member, the OU-noise actor: the deterministic kernel with
//                                  `constexpr bool OU = true`, which takes `ow` (ActorOuW) after the family's operands
//     FG_ACTOR_CATK (optional)     the name of the family's fourth member, the categorical actor: the deterministic kernel
//                                  with `constexpr bool CAT = true`, which takes `cw` (ActorCatW) after the family's operands
//     FG_ACTOR_SMP16, FG_ACTOR_CAT16 (optional, together)
//                                  the names of the family's 16-bit members: the Gaussian and the categorical kernel with
//                                  `constexpr bool OBS16 = true`, whose stream phase stores the observations as fp16 / bf16
//                                  units (write_obs16) in the format `obs_fmt`, the last kernel argument
// and they are undefined again here.  Not a header: no guard.  The body stays a textual include in each kernel
// (fg_actor_rollout_body.inc says why), so a kernel's token stream is what its hand-written wrapper was.
template <int NC, int H>
__global__ __launch_bounds__(FG_ACTOR_THREADS) void FG_ACTOR_DET(const Args a, FG_ACTOR_OPERANDS) {
    constexpr bool SAMPLE = false, OU = false, CAT = false, OBS16 = false, FG_ACTOR_FLAGS;
    constexpr int obs_fmt = 0;
    FG_ACTOR_ABSENT FG_ACTOR_NO_OW FG_ACTOR_NO_CW
    const float* const log_std = nullptr;
    float* const logp = nullptr;
#include "fg_actor_rollout_body.inc"
}

// log_std [2] read in place, log-probs to logp [K][B][N] when it is not NULL
template <int NC, int H>
__global__ __launch_bounds__(FG_ACTOR_THREADS) void FG_ACTOR_SMP(const Args a, FG_ACTOR_OPERANDS, const float* log_std,
                                                                 float* logp) {
    constexpr bool SAMPLE = true, OU = false, CAT = false, OBS16 = false, FG_ACTOR_FLAGS;
    constexpr int obs_fmt = 0;
    FG_ACTOR_ABSENT FG_ACTOR_NO_OW FG_ACTOR_NO_CW
#include "fg_actor_rollout_body.inc"
}

// the OU-noise actor: no log_std, no log-probs; the noise state ow.state [B][N][2] read at launch start, written at the end
#ifdef FG_ACTOR_OUK
template <int NC, int H>
__global__ __launch_bounds__(FG_ACTOR_THREADS) void FG_ACTOR_OUK(const Args a, FG_ACTOR_OPERANDS, const ActorOuW ow) {
    constexpr bool SAMPLE = false, OU = true, CAT = false, OBS16 = false, FG_ACTOR_FLAGS;
    constexpr int obs_fmt = 0;
    FG_ACTOR_ABSENT FG_ACTOR_NO_CW
    const float* const log_std = nullptr;
    float* const logp = nullptr;
#include "fg_actor_rollout_body.inc"
}
#undef FG_ACTOR_OUK
#endif

// the categorical actor: no log_std; indices to cw.idx [K][B][N], log-probs to cw.logp [K][B][N] when it is not NULL
#ifdef FG_ACTOR_CATK
template <int NC, int H>
__global__ __launch_bounds__(FG_ACTOR_THREADS) void FG_ACTOR_CATK(const Args a, FG_ACTOR_OPERANDS, const ActorCatW cw) {
    constexpr bool SAMPLE = false, OU = false, CAT = true, OBS16 = false, FG_ACTOR_FLAGS;
    constexpr int obs_fmt = 0;
    FG_ACTOR_ABSENT FG_ACTOR_NO_OW
    const float* const log_std = nullptr;
    float* const logp = nullptr;
#include "fg_actor_rollout_body.inc"
}
#undef FG_ACTOR_CATK
#endif

// the 16-bit members: a.obs holds 32-bit units (x | y << 16), a.obs_pitch counts them; obs_fmt: FG_WR_OBS_F16 / FG_WR_OBS_BF16
#ifdef FG_ACTOR_SMP16
template <int NC, int H>
__global__ __launch_bounds__(FG_ACTOR_THREADS) void FG_ACTOR_SMP16(const Args a, FG_ACTOR_OPERANDS, const float* log_std,
                                                                   float* logp, const int obs_fmt) {
    constexpr bool SAMPLE = true, OU = false, CAT = false, OBS16 = true, FG_ACTOR_FLAGS;
    FG_ACTOR_ABSENT FG_ACTOR_NO_OW FG_ACTOR_NO_CW
#include "fg_actor_rollout_body.inc"
}
template <int NC, int H>
__global__ __launch_bounds__(FG_ACTOR_THREADS) void FG_ACTOR_CAT16(const Args a, FG_ACTOR_OPERANDS, const ActorCatW cw,
                                                                   const int obs_fmt) {
    constexpr bool SAMPLE = false, OU = false, CAT = true, OBS16 = true, FG_ACTOR_FLAGS;
    FG_ACTOR_ABSENT FG_ACTOR_NO_OW
    const float* const log_std = nullptr;
    float* const logp = nullptr;
#include "fg_actor_rollout_body.inc"
}
#undef FG_ACTOR_SMP16
#undef FG_ACTOR_CAT16
#endif

#undef FG_ACTOR_DET
#undef FG_ACTOR_SMP
#undef FG_ACTOR_FLAGS
#undef FG_ACTOR_OPERANDS
#undef FG_ACTOR_ABSENT
