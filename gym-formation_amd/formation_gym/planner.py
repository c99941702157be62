"""A ready-made MPPI controller on `MultiAgentEnv.rollout_returns`, the way the env carries `get_action_BFS`.

Every control step a sampling planner draws C candidate action sequences around its nominal plan, scores them from the
current state and averages them, weighted by their returns, into the next plan.  The candidates are nothing more than
clamp(mean + sigma eps) with eps a pure function of (seed, env, candidate, agent, counter offset) - the library's counter RNG
on a stream of its own - so the [C, K, B, N, 2] tensor need not exist: the scoring launch draws each action where it uses it
(`fg_rollout_hd_returns_sampled`) and the update draws the same numbers again (`fg_plan_mppi_update`).

    planner = formation_gym.MPPIPlanner(env, horizon=20, candidates=8, sigma=0.5, lam=1.0)
    for t in range(T):
        action, info = planner.plan()               # [B, N, 2]; the env is left exactly where it was
        obs, rew, done, _ = env.step(action)
        planner.reset(done[:, 0])                   # (with auto_reset: a fresh episode starts from a zero plan)
"""
import math
import numbers

import torch

from . import _native

_MASK64 = (1 << 64) - 1


def _real(name, v, ok):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(float(v)) or not ok(float(v)):
        raise ValueError("MPPIPlanner: bad %s %r" % (name, v))
    return float(v)


class MPPIPlanner(object):
    """Model-predictive path integral control of a continuous-action env (a discrete action mode raises ValueError).

    horizon K >= 1 steps, candidates 1 <= C <= 2^17 per env, exploration `sigma` >= 0 (one value for every step, agent and
    component), temperature `lam` > 0, discount `gamma` in [0, 1], `clip` > 0: candidates are clamped to [-clip, clip]
    (clip <= 0: no clamp).  `sigma`, `lam`, `clip` and `gamma` are plain attributes, read (and checked) at every call.
    `noise_offset` is the planner's OWN counter: step k of a call draws at noise_offset + k, and `plan()` advances it by K, so
    that a plan made one env step later never re-draws the previous plan's noise shifted by one.  It is not the env's RNG
    offset: planning leaves the env's RNG, like everything else of the env, where it was.

    The planner owns `mean` [K, B, N, 2] (zeros at first) and a second buffer the update writes into; `plan()` swaps them.
    """

    def __init__(self, env, horizon, candidates, sigma, lam, gamma=1.0, clip=1.0, noise_offset=0):
        if env._action_mode():
            raise ValueError("MPPIPlanner needs a continuous-action env (no discrete_action_input / discrete_action_space / "
                             "force_discrete_action)")
        for name, v, hi in (("horizon", horizon, None), ("candidates", candidates, _native.PLAN_MAX_C)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1 or (hi and v > hi):
                raise ValueError("MPPIPlanner: bad %s %r" % (name, v))
        if env.num_agents > _native.PLAN_MAX_N:
            raise ValueError("MPPIPlanner: at most %d agents" % _native.PLAN_MAX_N)
        if isinstance(noise_offset, bool) or not isinstance(noise_offset, numbers.Integral) or not 0 <= noise_offset <= _MASK64:
            raise ValueError("MPPIPlanner: noise_offset must be an integer in [0, 2^64)")
        self.env = env
        self.horizon, self.num_candidates = int(horizon), int(candidates)
        self.sigma, self.lam, self.gamma, self.clip = sigma, lam, gamma, clip
        self.noise_offset = int(noise_offset)
        self._scalars()
        shape = (self.horizon, env.num_envs, env.num_agents, 2)
        dev = env.world.device
        self.mean = torch.zeros(shape, dtype=torch.float32, device=dev)
        self._spare = torch.zeros(shape, dtype=torch.float32, device=dev)
        self._launches, self._out = {}, None               # the fused route's bound launches and their result buffers

    def _scalars(self):
        """(sigma, lam, gamma, clip) as they are now, checked."""
        return (_real("sigma", self.sigma, lambda v: v >= 0.0), _real("lam", self.lam, lambda v: v > 0.0),
                _real("gamma", self.gamma, lambda v: 0.0 <= v <= 1.0), _real("clip", self.clip, lambda v: True))

    def path(self):
        """'fused' where `env.returns_path()` is: two launches per plan, no candidate tensor.  Else 'materialised':
        `fg_plan_candidates`, `env.rollout_returns` on that tensor (every scenario, agent count and World option it covers),
        `fg_plan_mppi_update`.  Decided without touching the device."""
        return "fused" if self.env.returns_path() == "fused" else "materialised"

    def _params(self):
        """The FgParams the element-wise planner launches read: the scenario's seed and the env's global index base."""
        sc = self.env.scenario
        p = self.env.world.native_params(seed=getattr(sc, "_seed", 0), scripted_ok=True)
        p.env_index_base = int(getattr(sc, "env_base", 0))
        return p

    def _dims(self):
        return self.env.num_envs, self.env.num_agents, self.horizon, self.num_candidates

    def candidates(self, noise_offset=None):
        """The [C, K, B, N, 2] candidates of the next `plan()` - or of the call at `noise_offset` - around the current `mean`
        (`fg_plan_candidates`): what the fused route draws without storing.  A fresh tensor."""
        sigma, _, _, clip = self._scalars()
        B, N, K, C = self._dims()
        off = self.noise_offset if noise_offset is None else int(noise_offset)
        dev = self.env.world.device
        out = torch.empty((C, K, B, N, 2), dtype=torch.float32, device=dev)
        _native.check(_native.load().fg_plan_candidates(self._params(), B, N, K, C, off & _MASK64, sigma, clip,
                                                        self.mean.data_ptr(), out.data_ptr(), _native.current_stream(dev)))
        return out

    def _score(self, off, sigma, gamma, clip):
        """(returns [C, B, N] as `rollout_returns` chooses them, info) of the candidates at offset `off`."""
        env = self.env
        if self.path() != "fused":
            return env.rollout_returns(self.candidates(off), gamma)
        launch, out = self._bound(gamma)
        launch(off, sigma, clip)
        return (out["ret"] if env.shared_reward else out["indiv"]), {"individual_return": out["indiv"], "steps": out["steps"]}

    def _bound(self, gamma):
        """(launch, out) of the fused scoring launch reading the current `mean`.  A binding holds an FgParams built when it was
        made, so it is keyed by everything that struct and the pointers depend on - the plan buffer, gamma, the world's physics
        constants (`World.params_signature()`, the rule of `_bound_step`), what `Scenario.params` reads of the scenario (seed,
        index base), the state tensors and the stream: a change of any of them binds again, as `rollout_returns`, which
        builds its params per call, sees it at once.  `out` - ret, indiv [C, B, N], steps [B] - is the planner's own, shared by
        its bindings; it is allocated once because B, N, K and C are fixed at construction (as are `mean`'s shapes)."""
        env = self.env
        w, sc = env.world, env.scenario
        dev = w.device
        key = (self.mean.data_ptr(), gamma, w.params_signature(), getattr(sc, "_seed", 0), getattr(sc, "env_base", 0),
               _native.current_stream(dev)) \
            + tuple(t.data_ptr() for t in (w.pos_x, w.pos_y, w.vel_x, w.vel_y, sc.ideal_shape, sc.ideal_vel, w.step_count))
        hit = self._launches.get(key)
        if hit is None:
            B, N, K, C = self._dims()
            if self._out is None:
                self._out = dict(ret=torch.empty((C, B, N), dtype=torch.float32, device=dev),
                                 indiv=torch.empty((C, B, N), dtype=torch.float32, device=dev),
                                 steps=torch.empty((B,), dtype=torch.int32, device=dev))
            if len(self._launches) >= 8:                       # stale keys (a constant, seed, stream or gamma that changed): start
                self._launches.clear()                         # anew - the other plan buffer's binding is made again on its turn
            hit = self._launches[key] = sc.bind_rollout_returns_sampled(w, self.mean, C, self._out, gamma)
        return hit, self._out

    def _update(self, off, sigma, clip, lam, returns, shift):
        """`fg_plan_mppi_update` from `mean` into the spare buffer: the action [B, N, 2] of step 0."""
        B, N, K, C = self._dims()
        dev = self.env.world.device
        ret = returns if returns.is_contiguous() else returns.contiguous()
        action = torch.empty((B, N, 2), dtype=torch.float32, device=dev)
        _native.check(_native.load().fg_plan_mppi_update(self._params(), B, N, K, C, off, sigma, clip, lam, ret.data_ptr(),
                                                         self.mean.data_ptr(), self._spare.data_ptr(), action.data_ptr(),
                                                         1 if shift else 0, _native.current_stream(dev)))
        return action

    def plan(self, shift=True):
        """One control step: score the C candidates around `mean` from the env's current state, weigh them
        (w_c = exp((R_c - max R) / lam) per (env, agent) on the returns `rollout_returns` gives) and average them into the
        next plan.  Returns (action [B, N, 2] - step 0 of the averaged plan -, info = {'returns' [C, B, N],
        'individual_return' [C, B, N], 'steps' [B], 'noise_offset': the offset this call drew at}).  With `shift` the new
        plan starts one step on (its last step repeated): the receding horizon; without, it stays aligned with this call.
        Advances `noise_offset` by K.  The env is left exactly as `rollout_returns` leaves it.  On the fused route the
        tensors in `info` are the planner's own buffers, as `step`'s results are the env's: the next `plan()` overwrites
        them - clone what must outlive it."""
        sigma, lam, gamma, clip = self._scalars()
        off = self.noise_offset & _MASK64
        returns, info = self._score(off, sigma, gamma, clip)
        action = self._update(off, sigma, clip, lam, returns, shift)
        self.mean, self._spare = self._spare, self.mean
        self.noise_offset = (off + self.horizon) & _MASK64
        return action, {"returns": returns, "individual_return": info["individual_return"], "steps": info["steps"],
                        "noise_offset": off}

    def reset(self, mask=None):
        """Zero the plan of the envs in `mask` (bool [B]; None: all of them), e.g. after their episode has ended."""
        if mask is None:
            self.mean.zero_()
        else:
            m = torch.as_tensor(mask, device=self.mean.device).to(torch.bool).reshape(-1)
            if m.numel() != self.mean.shape[1]:
                raise ValueError("mask must have one entry per env")
            self.mean.masked_fill_(m[None, :, None, None], 0.0)
