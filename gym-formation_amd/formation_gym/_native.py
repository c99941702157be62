"""ctypes binding of libformation_hip.so (C ABI: include/formation_hip.h).

The product path has NO CPU fallback: if the shared library is missing or a GPU
entry point fails, an exception is raised.  Pointers handed to the library are
`tensor.data_ptr()` of PyTorch-ROCm tensors; launches go to torch's current HIP
stream so torch events and stream semantics apply.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.path.join(_PKG_ROOT, "lib", "libformation_hip.so")
BUILD_SCRIPT = os.path.join(_PKG_ROOT, "csrc", "build.sh")

ABI_VERSION = 8
MAX_WALLS = 4
AGENT_PROPS = 8                 # floats per row of FgParams.agent_props: mass, size, accel, max_speed, u_noise, c_noise, flags, 0
AGENT_IMMOVABLE, AGENT_NO_COLLIDE, AGENT_GHOST, AGENT_SCRIPTED = 1, 2, 4, 8         # the flags column

FG_OK = 0
FG_ERR_BAD_ARG = -1
FG_ERR_UNSUPPORTED_N = -2
FG_ERR_ALIGNMENT = -3
FG_ERR_HIP = -4


class FgWall(ctypes.Structure):
    """Mirror of `struct FgWall`."""
    _fields_ = [("vertical", ctypes.c_int32), ("axis_pos", ctypes.c_float), ("end0", ctypes.c_float),
                ("end1", ctypes.c_float), ("width", ctypes.c_float), ("soft", ctypes.c_int32)]


class FgParams(ctypes.Structure):
    """Mirror of `struct FgParams` (include/formation_hip.h)."""
    _fields_ = [
        ("dt", ctypes.c_float),
        ("damping", ctypes.c_float),
        ("contact_force", ctypes.c_float),
        ("contact_margin", ctypes.c_float),
        ("sensitivity", ctypes.c_float),
        ("mass", ctypes.c_float),
        ("dist_min", ctypes.c_float),
        ("collide_thresh", ctypes.c_float),
        ("world_length", ctypes.c_int32),
        ("auto_reset", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
        ("rng_offset", ctypes.c_uint64),
        ("accel", ctypes.c_float),
        ("max_speed", ctypes.c_float),
        ("u_noise", ctypes.c_float),
        ("num_walls", ctypes.c_int32),
        ("walls", FgWall * 4),
        ("obs_env_pitch", ctypes.c_int32),
        ("env_index_base", ctypes.c_int32),
        ("rng_offset_dev", ctypes.c_void_p),
        ("agent_props", ctypes.c_void_p),       # device float [N][AGENT_PROPS] or NULL (uniform agents)
        ("comm_state", ctypes.c_void_p),        # device float [B][N][2] or NULL (silent agents)
        ("obs_placed", ctypes.c_int32),         # 1: the observation buffer was composed with fg_arena_* (placement.py)
        ("obs_zero_primed", ctypes.c_int32),    # 1: the zero blocks of the fp32 observation buffer already hold zeros (placement.py)
    ]


FG_SCN_BASIC, FG_SCN_PARTIAL, FG_SCN_RANGE, FG_SCN_OBSTACLE = 1, 2, 3, 4
FG_ACT_ONEHOT5, FG_ACT_INDEX, FG_ACT_ARGMAX = 1, 2, 3          # fg_decode_actions modes
FG_OBS_F16, FG_OBS_BF16 = 1, 2                                 # obs_format of fg_rollout_hd_obs16 / fg_rollout_hd_policy_obs16


def obs_format(dtype):
    """FG_OBS_* of a torch 16-bit float dtype; 0 for None (fp32 observations); ValueError for anything else."""
    import torch
    if dtype is None:
        return 0
    if dtype == torch.float16:
        return FG_OBS_F16
    if dtype == torch.bfloat16:
        return FG_OBS_BF16
    raise ValueError("obs_dtype must be None, torch.float16 or torch.bfloat16; got %r" % (dtype,))


class FgScenario(ctypes.Structure):
    """Mirror of `struct FgScenario` (include/formation_hip.h)."""
    _fields_ = [
        ("kind", ctypes.c_int32),
        ("num_landmarks", ctypes.c_int32),
        ("num_obstacles", ctypes.c_int32),
        ("num_obs", ctypes.c_int32),
        ("obs_range", ctypes.c_float),
        ("obstacle_size", ctypes.c_float),
        ("obstacle_vx", ctypes.c_float),
        ("obstacle_vy", ctypes.c_float),
        ("obstacle_floor", ctypes.c_float),
        ("penalty", ctypes.c_float),
        ("variant", ctypes.c_int32),            # 0 = library's choice, 1 = the run-time-count kernel
        ("reserved", ctypes.c_int32),
    ]


class FgActor(ctypes.Structure):
    """Mirror of `struct FgActor` (include/formation_hip.h): the caller's MLP actor for fg_rollout_hd_actor."""
    _fields_ = [
        ("hidden", ctypes.c_int32),
        ("out_tanh", ctypes.c_int32),
        ("w1", ctypes.c_void_p), ("b1", ctypes.c_void_p),
        ("w2", ctypes.c_void_p), ("b2", ctypes.c_void_p),
        ("w3", ctypes.c_void_p), ("b3", ctypes.c_void_p),
    ]


class FgActorNorm(ctypes.Structure):
    """Mirror of `struct FgActorNorm` (include/formation_hip.h): the LayerNorms of fg_rollout_hd_actor_norm's actor."""
    _fields_ = [
        ("in_gamma", ctypes.c_void_p), ("in_beta", ctypes.c_void_p),
        ("h1_gamma", ctypes.c_void_p), ("h1_beta", ctypes.c_void_p),
        ("h2_gamma", ctypes.c_void_p), ("h2_beta", ctypes.c_void_p),
        ("in_eps", ctypes.c_float), ("h1_eps", ctypes.c_float), ("h2_eps", ctypes.c_float),
        ("in_norm", ctypes.c_int32),            # 1: the actor starts with a LayerNorm over its input
    ]


def actor_norm(norms):
    """FgActorNorm of an `actor_rollout.ActorNorms`: (weight, bias, eps) of the input norm (None: absent) and of the two
    hidden norms; a None tensor is a NULL pointer (weight 1, bias 0)."""
    n0, n1, n2 = norms
    g0, b0, e0 = n0 if n0 is not None else (None, None, 1e-5)        # in_norm = 0: never read
    return FgActorNorm(ptr(g0), ptr(b0), ptr(n1[0]), ptr(n1[1]), ptr(n2[0]), ptr(n2[1]), e0, n1[2], n2[2],
                       0 if n0 is None else 1)


class FgActorGru(ctypes.Structure):
    """Mirror of `struct FgActorGru` (include/formation_hip.h): the recurrent layer of fg_rollout_hd_actor_gru's actor and the
    LayerNorm after it."""
    _fields_ = [
        ("w_ih", ctypes.c_void_p), ("w_hh", ctypes.c_void_p),
        ("b_ih", ctypes.c_void_p), ("b_hh", ctypes.c_void_p),
        ("norm_gamma", ctypes.c_void_p), ("norm_beta", ctypes.c_void_p),
        ("norm_eps", ctypes.c_float),
    ]


def actor_gru(gru):
    """FgActorGru of an `actor_rollout.ActorGru`: the GRU's four parameter tensors and (weight, bias, eps) of the norm after
    it; a None norm tensor is a NULL pointer (weight 1, bias 0)."""
    g, b, eps = gru.norm
    return FgActorGru(ptr(gru.w_ih), ptr(gru.w_hh), ptr(gru.b_ih), ptr(gru.b_hh), ptr(g), ptr(b), eps)


class FgActorInBn(ctypes.Structure):
    """Mirror of `struct FgActorInBn` (include/formation_hip.h): the eval-mode input BatchNorm of fg_rollout_hd_actor_bn's actor."""
    _fields_ = [
        ("mean", ctypes.c_void_p), ("var", ctypes.c_void_p),
        ("gamma", ctypes.c_void_p), ("beta", ctypes.c_void_p),
        ("eps", ctypes.c_float),
    ]


def actor_in_bn(bn):
    """FgActorInBn of an `actor_rollout.ActorInBn` (running_mean, running_var, weight, bias, eps); a None weight / bias is a
    NULL pointer (1 / 0)."""
    mean, var, g, b, eps = bn
    return FgActorInBn(ptr(mean), ptr(var), ptr(g), ptr(b), eps)


def actor_structs(actor):
    """The structs of an `actor_rollout.FusedActor`, as the actor launches take them: (FgActor[members], FgActorNorm,
    FgActorGru, FgActorInBn[members]), None for a struct the actor has no part for.  Their non-NULL pointer fields and the
    log_std argument are, between them, the addresses of `actor.tensors()`."""
    fas = (FgActor * len(actor.members))(*[
        FgActor(int(actor.hidden), int(actor.out_tanh), *[ptr(t) for t in ws]) for ws in actor.members])
    norm = None if actor.norms is None else actor_norm(actor.norms)
    gru = None if actor.gru is None else actor_gru(actor.gru)
    bns = None
    if actor.in_bn is not None:
        members = list(actor.in_bn) if actor.per_agent else [actor.in_bn]
        bns = (FgActorInBn * len(members))(*[actor_in_bn(m) for m in members])
    return fas, norm, gru, bns


class FgActorOu(ctypes.Structure):
    """Mirror of `struct FgActorOu` (include/formation_hip.h): the OU exploration of fg_rollout_hd_actor_ou's actor."""
    _fields_ = [("theta", ctypes.c_float), ("mu", ctypes.c_float), ("sigma", ctypes.c_float), ("scale", ctypes.c_float),
                ("clip", ctypes.c_float)]


def actor_ou(ou, into=None):
    """FgActorOu of an `actor_rollout.OUNoiseActor`'s five scalars as they are now (clip None: +inf, no clamp); `into`: the
    struct to update in place - a bound launcher's, so that an annealed scale is seen by its next launch."""
    s = FgActorOu() if into is None else into
    s.theta, s.mu, s.sigma, s.scale = float(ou.theta), float(ou.mu), float(ou.sigma), float(ou.scale)
    s.clip = float("inf") if ou.clip is None else float(ou.clip)
    return s


class FormationHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libformation_hip: status %d: %s" % (code, msg))
        self.code = code


_P = ctypes.c_void_p
_I = ctypes.c_int
_PP = ctypes.POINTER(FgParams)

# name -> (restype, argtypes); every symbol include/formation_hip.h declares
SIGNATURES = {
    "fg_abi_version": (_I, []),
    "fg_last_error": (ctypes.c_char_p, []),
    "fg_launch_device": (_I, [_P, _P]),
    "fg_arena_create": (_I, [_I, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_uint64),
                             ctypes.POINTER(ctypes.c_uint32)]),
    "fg_arena_map": (_I, [_P, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32, ctypes.POINTER(_P)]),
    "fg_arena_unmap": (_I, [_P, _P]),
    "fg_arena_keep_window": (_I, [_P, _P, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(_P)]),
    "fg_arena_trim": (_I, [_P]),
    "fg_arena_retired_address_bytes": (ctypes.c_uint64, []),
    "fg_arena_destroy": (_I, [_P]),
    "fg_kernel_config": (_I, [_I, ctypes.POINTER(_I), ctypes.POINTER(_I), ctypes.POINTER(_I)]),
    "fg_describe_launch": (_I, [_PP, ctypes.POINTER(FgScenario), _I, _I, _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fg_step_hd_bytes": (ctypes.c_int64, [_I]),
    "fg_step_hd": (_I, [_PP, _I, _I] + [_P] * 16),
    "fg_step_hd_plan": (_I, [_PP, _I, _I] + [_P] * 16 + [ctypes.POINTER(ctypes.c_void_p)]),
    "fg_plan_launch": (_I, [_P, ctypes.c_uint64]),
    "fg_plan_destroy": (_I, [_P]),
    "fg_physics_step": (_I, [_PP, _I, _I] + [_P] * 6),
    "fg_observe_hd": (_I, [_PP, _I, _I] + [_P] * 15),
    "fg_rollout_hd": (_I, [_PP, _I, _I, _I] + [_P] * 12 + [_I, _P]),
    "fg_reset_hd": (_I, [_PP, _I, _I] + [_P] * 9),
    "fg_reset_hd_mt": (_I, [_I, _I] + [_P] * 11),
    "fg_reset_hd_mt_done": (_I, [_I, _I, _I] + [_P] * 10 + [ctypes.c_int64, _P]),
    "fg_reset_scenario_mt": (_I, [ctypes.POINTER(FgScenario), _I, _I, _P, _I] + [_P] * 10),
    "fg_step_basic": (_I, [_PP, _I, _I, _I, _I] + [_P] * 13),
    "fg_step_scenario": (_I, [_PP, ctypes.POINTER(FgScenario), _I, _I, _I] + [_P] * 14),
    "fg_reset_scenario": (_I, [_PP, ctypes.POINTER(FgScenario), _I, _I] + [_P] * 10),
    "fg_rollout_scenario": (_I, [_PP, ctypes.POINTER(FgScenario), _I, _I, _I] + [_P] * 14 + [_I, _P]),
    "fg_decode_actions": (_I, [_I, ctypes.c_int64, _P, _P, _P]),
    "fg_update_comm": (_I, [_PP, _I, _I, _P, _P, _P]),
    "fg_update_comm_dim": (_I, [_PP, _I, _I, _I, _P, _P, _P]),
    "fg_policy_bfs": (_I, [_I, _I, _I, _P, ctypes.c_int64, _P, _P]),
    "fg_policy_bfs_state": (_I, [_I, _I, _I] + [_P] * 6),
    "fg_rollout_hd_policy": (_I, [_PP, _I, _I, _I, _I] + [_P] * 12 + [_I, _P]),
    "fg_rollout_hd_obs16": (_I, [_PP, _I, _I, _I, _I] + [_P] * 12 + [_I, _P]),
    "fg_rollout_hd_policy_obs16": (_I, [_PP, _I, _I, _I, _I, _I] + [_P] * 12 + [_I, _P]),
    "fg_describe_obs16_launch": (_I, [_PP, _I, _I, _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fg_rollout_hd_actor": (_I, [_PP, ctypes.POINTER(FgActor), _I, _I, _I] + [_P] * 12 + [_I, _P]),
    "fg_describe_actor_launch": (_I, [_PP, ctypes.POINTER(FgActor), _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fg_rollout_hd_actor_sample": (_I, [_PP, ctypes.POINTER(FgActor), _P, _I, _I, _I] + [_P] * 13 + [_I, _P]),
    "fg_actor_noise": (_I, [_PP, _I, _I, _P, _P]),
    "fg_actor_log_prob": (_I, [_P, _P, ctypes.c_int64, _P, _P]),
    "fg_describe_actor_sample_launch": (_I, [_PP, ctypes.POINTER(FgActor), _P, _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fg_rollout_hd_actor_per_agent": (_I, [_PP, ctypes.POINTER(FgActor), _P, _I, _I, _I] + [_P] * 13 + [_I, _P]),
    "fg_describe_actor_per_agent_launch": (_I, [_PP, ctypes.POINTER(FgActor), _P, _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fg_rollout_hd_actor_norm": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorNorm), _P, _I, _I, _I] + [_P] * 13
                                 + [_I, _P]),
    "fg_describe_actor_norm_launch": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorNorm), _P, _I, _I, _I, _I,
                                           ctypes.c_char_p, _I]),
    "fg_rollout_hd_actor_gru": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorNorm), ctypes.POINTER(FgActorGru), _P,
                                     _I, _I, _I] + [_P] * 14 + [_I, _P]),
    "fg_rollout_hd_actor_gru_states": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorNorm),
                                            ctypes.POINTER(FgActorGru), _P, _I, _I, _I] + [_P] * 15 + [_I, _I, _P]),
    "fg_describe_actor_gru_launch": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorNorm), ctypes.POINTER(FgActorGru),
                                          _P, _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fg_rollout_hd_actor_bn": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorInBn), _P, _I, _I, _I] + [_P] * 13
                               + [_I, _P]),
    "fg_rollout_hd_actor_bn_per_agent": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorInBn), _P, _I, _I, _I]
                                         + [_P] * 13 + [_I, _P]),
    "fg_describe_actor_bn_launch": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorInBn), _P, _I, _I, _I, _I,
                                         ctypes.c_char_p, _I]),
    "fg_describe_actor_bn_per_agent_launch": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorInBn), _P, _I, _I, _I, _I,
                                                   ctypes.c_char_p, _I]),
    "fg_rollout_hd_actor_ou": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorInBn), ctypes.POINTER(FgActorOu), _P,
                                    _I, _I, _I] + [_P] * 12 + [_I, _P]),
    "fg_rollout_hd_actor_ou_per_agent": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorInBn),
                                              ctypes.POINTER(FgActorOu), _P, _I, _I, _I] + [_P] * 12 + [_I, _P]),
    "fg_describe_actor_ou_launch": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorInBn), ctypes.POINTER(FgActorOu),
                                         _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fg_describe_actor_ou_per_agent_launch": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorInBn),
                                                   ctypes.POINTER(FgActorOu), _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fg_actor_ou_step": (_I, [ctypes.POINTER(FgActorOu), ctypes.c_int64, _P, _P, _P]),
    "fg_rollout_hd_actor_cat": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorNorm), ctypes.POINTER(FgActorGru),
                                     _I, _I, _I, _I, _I] + [_P] * 16 + [_I, _I, _P]),
    "fg_describe_actor_cat_launch": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorNorm), ctypes.POINTER(FgActorGru),
                                          _I, _I, _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fg_rollout_hd_actor_obs16": (_I, [_PP, _I, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorNorm), ctypes.POINTER(FgActorGru),
                                       _P, _I, _I, _I] + [_P] * 15 + [_I, _I, _P]),
    "fg_describe_actor_obs16_launch": (_I, [_PP, _I, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorNorm),
                                            ctypes.POINTER(FgActorGru), _P, _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fg_rollout_hd_actor_cat_obs16": (_I, [_PP, _I, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorNorm),
                                           ctypes.POINTER(FgActorGru), _I, _I, _I, _I, _I] + [_P] * 16 + [_I, _I, _P]),
    "fg_describe_actor_cat_obs16_launch": (_I, [_PP, _I, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorNorm),
                                                ctypes.POINTER(FgActorGru), _I, _I, _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fg_actor_uniform": (_I, [_PP, _I, _I, _P, _P]),
    "fg_actor_categorical": (_I, [_I, _I, ctypes.c_int64, _P, _P, _P, _P, _P, _P]),
    "fg_rollout_hd_actor_gumbel": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorInBn), _I, _I, _I, _I, _I] + [_P] * 13
                                   + [_I, _P]),
    "fg_rollout_hd_actor_gumbel_per_agent": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorInBn), _I, _I, _I, _I, _I]
                                             + [_P] * 13 + [_I, _P]),
    "fg_describe_actor_gumbel_launch": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorInBn), _I, _I, _I, _I, _I, _I,
                                             ctypes.c_char_p, _I]),
    "fg_describe_actor_gumbel_per_agent_launch": (_I, [_PP, ctypes.POINTER(FgActor), ctypes.POINTER(FgActorInBn), _I, _I, _I, _I, _I,
                                                       _I, ctypes.c_char_p, _I]),
    "fg_actor_gumbel": (_I, [_PP, _I, _I, _P, _P]),
    "fg_actor_gumbel_pick": (_I, [_I, _I, ctypes.c_int64, _P, _P, _P, _P, _P]),
    "fg_rollout_scenario_actor": (_I, [_PP, ctypes.POINTER(FgScenario), ctypes.POINTER(FgActor), _P, _I, _I, _I] + [_P] * 14
                                  + [_I, _P]),
    "fg_describe_scenario_actor_launch": (_I, [_PP, ctypes.POINTER(FgScenario), ctypes.POINTER(FgActor), _P, _I, _I, _I, _I,
                                               ctypes.c_char_p, _I]),
    "fg_rollout_hd_returns": (_I, [_PP, _I, _I, _I, _I, ctypes.c_float] + [_P] * 12),
    "fg_describe_returns_launch": (_I, [_PP, _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fg_rollout_hd_returns_sampled": (_I, [_PP, _I, _I, _I, _I, ctypes.c_float, ctypes.c_uint64, ctypes.c_float, ctypes.c_float]
                                      + [_P] * 12),
    "fg_describe_returns_sampled_launch": (_I, [_PP, _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fg_plan_candidates": (_I, [_PP, _I, _I, _I, _I, ctypes.c_uint64, ctypes.c_float, ctypes.c_float, _P, _P, _P]),
    "fg_plan_mppi_update": (_I, [_PP, _I, _I, _I, _I, ctypes.c_uint64, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                 _P, _P, _P, _P, _I, _P]),
    "fg_plan_candidates_std": (_I, [_PP, _I, _I, _I, _I, ctypes.c_uint64, ctypes.c_float, _P, _P, _P, _P]),
    "fg_rollout_hd_returns_sampled_std": (_I, [_PP, _I, _I, _I, _I, ctypes.c_float, ctypes.c_uint64, ctypes.c_float] + [_P] * 13),
    "fg_describe_returns_sampled_std_launch": (_I, [_PP, _I, _I, _I, _I, ctypes.c_char_p, _I]),
    "fg_plan_cem_update": (_I, [_PP, _I, _I, _I, _I, _I, ctypes.c_uint64, ctypes.c_float, ctypes.c_float, ctypes.c_float]
                           + [_P] * 7 + [_I, _P]),
}
PLAN_MAX_N, PLAN_MAX_C = 1 << 12, 1 << 17         # a planner's agent and candidate counts (the stream code's fields)
# fg_plan_cem_update's two thresholds (fg_planner_kernels.hpp: FG_CEM_REG_C, FG_CEM_ELITE_CAP): up to CEM_REG_C candidates a
# row's keys stay in registers, up to CEM_ELITE_CAP elites a row's elite list is kept in LDS
CEM_REG_C, CEM_ELITE_CAP = 4096, 1024

_lib = None


def build(force=False):
    """Compile the HIP library in-tree (hipcc --offload-arch=gfx950)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(["bash", BUILD_SCRIPT])
    return LIB_PATH


def load():
    """Load the library, set prototypes, check the ABI version.  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FormationHipError(
            FG_ERR_HIP, "%s not found - run gym-formation_amd/csrc/build.sh "
            "(there is no CPU fallback for the hot path)" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.fg_abi_version() != ABI_VERSION:
        raise FormationHipError(FG_ERR_BAD_ARG, "ABI version mismatch: library %d, binding %d"
                                % (lib.fg_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(code):
    if code != FG_OK:
        raise FormationHipError(code, load().fg_last_error().decode("utf-8", "replace"))


def bind_launch(fn, p, *args, keep=None):
    """`launch(rng_offset)` for a bound K-step launch: sets the FgParams struct `p`'s RNG offset, makes the ONE ctypes call
    `fn(p, *args)` with everything else resolved by the caller, raises on a non-zero status and returns `keep` - what the
    launch reads in place and must outlive it.  The closure is the only Python frame per launch."""
    def launch(rng_offset=0):
        p.rng_offset = rng_offset
        rc = fn(p, *args)
        if rc:
            check(rc)
        return keep
    return launch


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def current_stream(device=None):
    """Raw handle of torch's current stream ON `device` (the device the env's tensors live on, which need
    not be the process's current device: the library switches to the stream's device for the launch)."""
    import torch
    return torch.cuda.current_stream(device).cuda_stream


def current_stream_fast(device):
    """Raw handle of torch's current stream on `device` without building a Stream object
    (the per-step API path calls this on every step)."""
    import torch
    try:
        return torch._C._cuda_getCurrentRawStream(device.index if device.index is not None else torch.cuda.current_device())
    except AttributeError:                # private helper missing in this torch build
        return torch.cuda.current_stream(device).cuda_stream


def kernel_config(n):
    t, e, l = _I(), _I(), _I()
    check(load().fg_kernel_config(int(n), ctypes.byref(t), ctypes.byref(e), ctypes.byref(l)))
    return {"threads": t.value, "envs_per_wg": e.value, "lds_bytes": l.value}


def step_hd_bytes(n):
    return int(load().fg_step_hd_bytes(int(n)))
