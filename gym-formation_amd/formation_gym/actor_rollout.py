"""Which launch runs `env.rollout_actor(K, actor)`: the fused closed loop (`fg_rollout_hd_actor`, the actor evaluated inside
the rollout kernel) or the host-paced loop (`actor(obs); env.step(a)` in Python).

The fused kernel takes one actor shared by every agent, exactly
    torch.nn.Sequential(Linear(6N, H), ReLU(), Linear(H, H), ReLU(), Linear(H, 2) [, Tanh()])
with H in {32, 64, 128}, fp32 contiguous parameters on the env's device (a None bias counts as zero), for N in
{3, 4, 8, 9, 16, 25, 27, 32} agents of formation_hd_env with continuous actions, silent agents, no World options and no
post_step_callback.  Anything else runs host-paced: a shape or option the kernel cannot honour never runs fused."""
import torch

FUSED_N = (3, 4, 8, 9, 16, 25, 27, 32)
FUSED_HIDDEN = (32, 64, 128)


def actor_spec(actor, num_agents, device=None):
    """(hidden, out_tanh, [w1, b1, w2, b2, w3, b3]) when the fused kernel can evaluate `actor` for `num_agents` agents, else
    None.  `device`: the env's device (None: not checked).  The tensors are the actor's own parameters (b* may be None)."""
    nn = torch.nn
    if type(actor) is not nn.Sequential or int(num_agents) not in FUSED_N:
        return None
    mods = list(actor)
    kinds = [type(m) for m in mods]
    body = [nn.Linear, nn.ReLU, nn.Linear, nn.ReLU, nn.Linear]
    if kinds != body and kinds != body + [nn.Tanh]:
        return None
    l1, l2, l3 = mods[0], mods[2], mods[4]
    H = l1.out_features
    if H not in FUSED_HIDDEN or l1.in_features != 6 * int(num_agents) or (l2.in_features, l2.out_features) != (H, H) \
            or (l3.in_features, l3.out_features) != (H, 2):
        return None
    params = [l1.weight, l1.bias, l2.weight, l2.bias, l3.weight, l3.bias]
    dev = None if device is None else torch.device(device)
    for t in params:
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous():
            return None
        if dev is not None and (t.device.type != dev.type or (dev.index is not None and t.device.index != dev.index)):
            return None
    return H, len(mods) == 6, params


def actor_path(actor, num_agents, device=None, fused_scenario=True, continuous=True, silent=True, world_options=False,
               callback=False):
    """'fused' or 'host': the one decision `MultiAgentEnv.actor_path` / `rollout_actor` take.  The keyword facts describe the
    env: a scenario with the fused launch (formation_hd_env), continuous actions, silent agents, no World options (walls,
    accel, max_speed, u_noise, per-agent properties), no post_step_callback."""
    if not (fused_scenario and continuous and silent) or world_options or callback:
        return "host"
    return "fused" if actor_spec(actor, num_agents, device) is not None else "host"
