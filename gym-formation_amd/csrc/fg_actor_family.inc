// fg_actor_family.inc - one formation_hd_env actor family (fg_actor_rollout_kernel.hpp): the kernel of every member the family
// has, then the host's record of the family.  The family block that includes this file defines FG_ACTOR_KIND, FG_ACTOR_MAXH and
// FG_ACTOR_WHAT (its HdActorKind, the widest H it is built for, its word in a failed launch's text), FG_ACTOR_FLAGS (its
// ActorFlags), FG_ACTOR_OPERANDS (the kernel parameters after `a`), FG_ACTOR_ABSENT (the FG_ACTOR_NO_* constants of the operands
// it does not take), FG_ACTOR_DET and FG_ACTOR_SMP (the names of the deterministic and the Gaussian member) and, where it has
// them, FG_ACTOR_OUK, FG_ACTOR_CATK, FG_ACTOR_GUMK and - together - FG_ACTOR_SMP16 and FG_ACTOR_CAT16 (the OU, categorical, Gumbel
// and 16-bit members); they are undefined again here.  A wrapper is its member (FG_ACTOR_IS: the body's flags, from the predicates the
// host sizes the LDS with), the member's kernel parameters after the family's operands, and the stand-ins for the ones it lacks.
// Not a header: no guard.  The body stays a textual include in each kernel (fg_actor_rollout_body.inc says why).
template <int NC, int H>
__global__ __launch_bounds__(FG_ACTOR_THREADS) void FG_ACTOR_DET(const Args a, FG_ACTOR_OPERANDS) {
    FG_ACTOR_IS(ACTOR_DET) FG_ACTOR_NO_GAUSS FG_ACTOR_NO_OW FG_ACTOR_NO_CW FG_ACTOR_NO_OBS16 FG_ACTOR_NO_GUM
#include "fg_actor_rollout_body.inc"
}
// log_std [2] read in place, log-probs to logp [K][B][N] when it is not NULL
template <int NC, int H>
__global__ __launch_bounds__(FG_ACTOR_THREADS) void FG_ACTOR_SMP(const Args a, FG_ACTOR_OPERANDS, const float* log_std,
                                                                 float* logp) {
    FG_ACTOR_IS(ACTOR_GAUSS) FG_ACTOR_NO_OW FG_ACTOR_NO_CW FG_ACTOR_NO_OBS16 FG_ACTOR_NO_GUM
#include "fg_actor_rollout_body.inc"
}
// no log_std, no log-probs; the noise state ow.state [B][N][2] read at launch start, written at the end
#ifdef FG_ACTOR_OUK
template <int NC, int H>
__global__ __launch_bounds__(FG_ACTOR_THREADS) void FG_ACTOR_OUK(const Args a, FG_ACTOR_OPERANDS, const ActorOuW ow) {
    FG_ACTOR_IS(ACTOR_OU) FG_ACTOR_NO_GAUSS FG_ACTOR_NO_CW FG_ACTOR_NO_OBS16 FG_ACTOR_NO_GUM
#include "fg_actor_rollout_body.inc"
}
#endif
// no log_std; indices to cw.idx [K][B][N], log-probs to cw.logp [K][B][N] when it is not NULL
#ifdef FG_ACTOR_CATK
template <int NC, int H>
__global__ __launch_bounds__(FG_ACTOR_THREADS) void FG_ACTOR_CATK(const Args a, FG_ACTOR_OPERANDS, const ActorCatW cw) {
    FG_ACTOR_IS(ACTOR_CAT) FG_ACTOR_NO_GAUSS FG_ACTOR_NO_OW FG_ACTOR_NO_OBS16 FG_ACTOR_NO_GUM
#include "fg_actor_rollout_body.inc"
}
#endif
// no log_std, no log-probs; indices to gum.idx [K][B][N]
#ifdef FG_ACTOR_GUMK
template <int NC, int H>
__global__ __launch_bounds__(FG_ACTOR_THREADS) void FG_ACTOR_GUMK(const Args a, FG_ACTOR_OPERANDS, const ActorGumW gum) {
    FG_ACTOR_IS(ACTOR_GUMBEL) FG_ACTOR_NO_GAUSS FG_ACTOR_NO_OW FG_ACTOR_NO_CW FG_ACTOR_NO_OBS16
#include "fg_actor_rollout_body.inc"
}
#endif
// the 16-bit members: a.obs holds 32-bit units (x | y << 16), a.obs_pitch counts them; obs_fmt: FG_WR_OBS_F16 / FG_WR_OBS_BF16
#ifdef FG_ACTOR_SMP16
template <int NC, int H>
__global__ __launch_bounds__(FG_ACTOR_THREADS) void FG_ACTOR_SMP16(const Args a, FG_ACTOR_OPERANDS, const float* log_std,
                                                                   float* logp, const int obs_fmt) {
    FG_ACTOR_IS(ACTOR_GAUSS16) FG_ACTOR_NO_OW FG_ACTOR_NO_CW FG_ACTOR_NO_GUM
#include "fg_actor_rollout_body.inc"
}
template <int NC, int H>
__global__ __launch_bounds__(FG_ACTOR_THREADS) void FG_ACTOR_CAT16(const Args a, FG_ACTOR_OPERANDS, const ActorCatW cw,
                                                                   const int obs_fmt) {
    FG_ACTOR_IS(ACTOR_CAT16) FG_ACTOR_NO_GAUSS FG_ACTOR_NO_OW FG_ACTOR_NO_GUM
#include "fg_actor_rollout_body.inc"
}
#endif

// The host's record (formation_hip.hip: launch_hd_member).  A member the block does not name has no name here, and `kernel` is
// asked only for a member that `has` answers for, so that nothing else is instantiated.
template <> struct HdActorFamily<FG_ACTOR_KIND> {
    static constexpr ActorFlags flags = FG_ACTOR_FLAGS;
    static constexpr int max_h = FG_ACTOR_MAXH;
    static constexpr const char* fail_fmt = FG_ACTOR_WHAT "actor rollout launch failed: %s";
    static constexpr const char* name(ActorMember m) {         // as the describe strings spell it; NULL: no such member
        switch (m) {
        case ACTOR_DET: return FG_ACTOR_STR(FG_ACTOR_DET);
        case ACTOR_GAUSS: return FG_ACTOR_STR(FG_ACTOR_SMP);
#ifdef FG_ACTOR_OUK
        case ACTOR_OU: return FG_ACTOR_STR(FG_ACTOR_OUK);
#endif
#ifdef FG_ACTOR_CATK
        case ACTOR_CAT: return FG_ACTOR_STR(FG_ACTOR_CATK);
#endif
#ifdef FG_ACTOR_SMP16
        case ACTOR_GAUSS16: return FG_ACTOR_STR(FG_ACTOR_SMP16);
        case ACTOR_CAT16: return FG_ACTOR_STR(FG_ACTOR_CAT16);
#endif
#ifdef FG_ACTOR_GUMK
        case ACTOR_GUMBEL: return FG_ACTOR_STR(FG_ACTOR_GUMK);
#endif
        default: return nullptr;
        }
    }
    static constexpr bool has(ActorMember m, int n, int h) { return name(m) && (!actor_member_obs16(m) || actor_obs16_shape(n, h)); }
    template <ActorMember M, int NC, int H> static constexpr auto kernel() {
        if constexpr (M == ACTOR_DET) return &FG_ACTOR_DET<NC, H>; else if constexpr (M == ACTOR_GAUSS) return &FG_ACTOR_SMP<NC, H>;
#ifdef FG_ACTOR_OUK
        else if constexpr (M == ACTOR_OU) return &FG_ACTOR_OUK<NC, H>;
#endif
#ifdef FG_ACTOR_CATK
        else if constexpr (M == ACTOR_CAT) return &FG_ACTOR_CATK<NC, H>;
#endif
#ifdef FG_ACTOR_SMP16
        else if constexpr (M == ACTOR_GAUSS16) return &FG_ACTOR_SMP16<NC, H>;
        else if constexpr (M == ACTOR_CAT16) return &FG_ACTOR_CAT16<NC, H>;
#endif
#ifdef FG_ACTOR_GUMK
        else if constexpr (M == ACTOR_GUMBEL) return &FG_ACTOR_GUMK<NC, H>;
#endif
    }
};

#undef FG_ACTOR_KIND
#undef FG_ACTOR_MAXH
#undef FG_ACTOR_WHAT
#undef FG_ACTOR_FLAGS
#undef FG_ACTOR_OPERANDS
#undef FG_ACTOR_ABSENT
#undef FG_ACTOR_DET
#undef FG_ACTOR_SMP
#undef FG_ACTOR_OUK
#undef FG_ACTOR_CATK
#undef FG_ACTOR_GUMK
#undef FG_ACTOR_SMP16
#undef FG_ACTOR_CAT16
