"""Helpers the actor test files share (tests/test_gpu_actor_*.py and tests/test_actor_*_cpu.py): the env and the actors the GPU
tests build, the bookkeeping around one `rollout_actor` call, and the stand-ins of the CPU tests' C ABI calls.  A plain module:
no fixtures, nothing registered with pytest.  The error models and measured figures stay in the test files' docstrings; they
rest on `env` and `scaled_mlp` building bit for bit what they build now."""
import ctypes
import os

import numpy as np
import torch

import formation_gym
from formation_gym import _native
from formation_gym.actor_rollout import LOG_2PI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gym-formation_amd", "lib", "libformation_hip.so")

DEV = "cuda:0"
B = 133                  # not a multiple of any workgroup's env count (8, 16, 32, 64; 256 in the landmark scenarios)
K = 24
ACT_SCALE = 1.5


# ---- GPU side ----
def env(N, seed=3, num_envs=B, name="formation_hd_env"):
    """`name` with N agents, seeded and reset, auto-resetting, with an episode boundary inside a K-step launch for a third of
    the envs."""
    e = formation_gym.make_env(name, False, N, num_envs=num_envs, device=DEV)
    e.seed(seed)
    e.reset()
    e.auto_reset = True
    wl = int(e.world.world_length)
    step0 = np.random.RandomState(seed).randint(0, wl, num_envs)
    step0[::3] = wl - 7
    e.world.step_count.copy_(torch.as_tensor(step0, dtype=torch.int32))
    return e


def scaled_mlp(D, H, tanh, seed=0, scale=ACT_SCALE):
    """Sequential(Linear(D, H), ReLU, Linear(H, H), ReLU, Linear(H, 2) [, Tanh]) on DEV: PyTorch's default initialisation under
    `seed`, every parameter multiplied by `scale`."""
    torch.manual_seed(seed)
    mods = [torch.nn.Linear(D, H), torch.nn.ReLU(), torch.nn.Linear(H, H), torch.nn.ReLU(), torch.nn.Linear(H, 2)]
    if tanh:
        mods.append(torch.nn.Tanh())
    m = torch.nn.Sequential(*mods).to(DEV)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(scale)
    return m


class Wrap(torch.nn.Module):
    """The same function behind a module the path rule does not recognise: runs host-paced."""

    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        return self.m(x)


def current_obs(e):
    obs = torch.empty_like(e._out["obs"])
    e.scenario.observe_batch(e.world, {"obs": obs})
    return obs


def state(e):
    """formation_hd_env's whole state, cloned (the landmark tests keep their own list)."""
    w, sc = e.world, e.scenario
    return [t.clone() for t in (w.pos_x, w.pos_y, w.vel_x, w.vel_y, w.step_count, sc.ideal_shape, sc.ideal_vel)]


def clone(res):
    obs, rew, done, info = res
    return obs.clone(), rew.clone(), done.clone(), {k: v.clone() for k, v in info.items()}


def obs_before(obs0, obs, K_):
    """The observation each of K_ steps acted on: obs0, then what the step before returned."""
    return [obs0] + [obs[k - 1] for k in range(1, K_)]


def noise_at(e, k):
    """fg_actor_noise at the offset of step k of the next launch."""
    sc = e.scenario
    p = e.world.native_params(seed=sc._seed, rng_offset=e._launch_rng_offset() + k)
    p.env_index_base = int(getattr(sc, "env_base", 0))
    eps = torch.empty((e.num_envs, e.num_agents, 2), dtype=torch.float32, device=DEV)
    _native.check(_native.load().fg_actor_noise(p, e.num_envs, e.num_agents, eps.data_ptr(), _native.current_stream(DEV)))
    return eps


def logp_formula(eps, log_std):
    return -0.5 * (eps[..., 0] * eps[..., 0] + eps[..., 1] * eps[..., 1]) - (log_std[0] + log_std[1]) - LOG_2PI


def hand_loop(e, actor, K_):
    """The host-paced loop by hand: (actions, observations, rewards) of K_ steps of `actor` from the current state."""
    obs = current_obs(e)
    acts, obss, rews = [], [], []
    with torch.no_grad():
        for _ in range(K_):
            a = actor(obs)
            acts.append(a.clone())
            obs, r, d, info = e.step(a)
            obss.append(obs.clone()); rews.append(r.clone())
    return torch.stack(acts), torch.stack(obss), torch.stack(rews)


# ---- CPU side: the C ABI without a device ----
def params(dist_min=0.06, collide_thresh=0.03, world_length=100):
    p = _native.FgParams()
    p.dt, p.damping, p.contact_force, p.contact_margin = 0.1, 0.25, 100.0, 0.001
    p.sensitivity, p.mass, p.dist_min, p.collide_thresh = 5.0, 1.0, dist_min, collide_thresh
    p.world_length = world_length
    return p


def fake_actor(H, tanh=1):
    addr = 4096                                       # stand-ins: only NULL-ness and alignment are looked at
    return _native.FgActor(H, tanh, addr, addr, addr, addr, addr, addr)


def fake_actors(N, H, tanh=1):
    """A host array of N fake_actor members, as the per-agent entries take it."""
    return (_native.FgActor * N)(*[fake_actor(H, tanh) for _ in range(N)])


def describe(lib, entry, lead, N, B=4096, K=20, p=None):
    """(status, text) of the dry run `entry` (an fg_describe_*actor*_launch symbol); `lead`: its arguments between the params
    and B (the scenario descriptor, the actor(s), the norms, log_std - whichever it takes)."""
    buf = ctypes.create_string_buffer(512)
    rc = getattr(lib, entry)(p or params(), *lead, B, N, K, 1, buf, 512)
    return rc, buf.value.decode()
