"""Ready-made MPPI and CEM controllers on `MultiAgentEnv.rollout_returns`, the way the env carries `get_action_BFS`.

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

`CEMPlanner` is the cross-entropy method on the same stream: a sigma per step, env, agent and component, refit with the mean to
each row's best candidates (`fg_rollout_hd_returns_sampled_std`, `fg_plan_cem_update`), again without the tensor.
"""
import math
import numbers

import torch

from . import _native

_MASK64 = (1 << 64) - 1


def _real(name, v, ok, who="MPPIPlanner"):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(float(v)) or not ok(float(v)):
        raise ValueError("%s: bad %s %r" % (who, name, v))
    return float(v)


class _SamplingPlanner(object):
    """What the sampling planners share: the checks of the constructor's integers, the plan buffers `mean` / `_spare`
    [K, B, N, 2], the route, the params of the element-wise launches, the cache of bound scoring launches and `reset`."""
    _WHO = "planner"

    def _setup(self, env, horizon, candidates, noise_offset):
        who = self._WHO
        if env._action_mode():
            raise ValueError("%s needs a continuous-action env (no discrete_action_input / discrete_action_space / "
                             "force_discrete_action)" % who)
        for name, v, hi in (("horizon", horizon, None), ("candidates", candidates, _native.PLAN_MAX_C)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1 or (hi and v > hi):
                raise ValueError("%s: bad %s %r" % (who, name, v))
        if env.num_agents > _native.PLAN_MAX_N:
            raise ValueError("%s: at most %d agents" % (who, _native.PLAN_MAX_N))
        if isinstance(noise_offset, bool) or not isinstance(noise_offset, numbers.Integral) or not 0 <= noise_offset <= _MASK64:
            raise ValueError("%s: noise_offset must be an integer in [0, 2^64)" % who)
        self.env = env
        self.horizon, self.num_candidates = int(horizon), int(candidates)
        self.noise_offset = int(noise_offset)

    def _plan_buffer(self):
        return torch.zeros((self.horizon, self.env.num_envs, self.env.num_agents, 2), dtype=torch.float32,
                           device=self.env.world.device)

    def path(self):
        """'fused' where `env.returns_path()` is: two launches per scoring-and-update round, no candidate tensor.  Else
        'materialised': the candidates as a tensor, `env.rollout_returns` on it (every scenario, agent count and World option
        it covers), the same update.  Decided without touching the device."""
        return "fused" if self.env.returns_path() == "fused" else "materialised"

    def _params(self):
        """The FgParams the element-wise planner launches read: the scenario's seed and the env's global index base."""
        sc = self.env.scenario
        p = self.env.world.native_params(seed=getattr(sc, "_seed", 0), scripted_ok=True)
        p.env_index_base = int(getattr(sc, "env_base", 0))
        return p

    def _dims(self):
        return self.env.num_envs, self.env.num_agents, self.horizon, self.num_candidates

    def _binding(self, buffers, extra, bind):
        """(launch, out) of the fused scoring launch reading the plan `buffers`.  A binding holds an FgParams built when it
        was made, so it is keyed by everything that struct and the pointers depend on - the plan buffers, `extra`, the world's
        physics constants (`World.params_signature()`, the rule of `_bound_step`), what `Scenario.params` reads of the scenario
        (seed, index base), the state tensors and the stream: a change of any of them binds again (`bind(out)`), as
        `rollout_returns`, which builds its params per call, sees it at once.  `out` - ret, indiv [C, B, N], steps [B] - is
        the planner's own, shared by its bindings; it is allocated once because B, N, K and C are fixed at construction."""
        env = self.env
        w, sc = env.world, env.scenario
        dev = w.device
        key = tuple(t.data_ptr() for t in buffers) + (extra, w.params_signature(), getattr(sc, "_seed", 0),
                                                      getattr(sc, "env_base", 0), _native.current_stream(dev)) \
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
            hit = self._launches[key] = bind(self._out)
        return hit, self._out

    def reset(self, mask=None):
        """Zero the plan of the envs in `mask` (bool [B]; None: all of them), e.g. after their episode has ended."""
        if mask is None:
            self.mean.zero_()
        else:
            m = torch.as_tensor(mask, device=self.mean.device).to(torch.bool).reshape(-1)
            if m.numel() != self.mean.shape[1]:
                raise ValueError("mask must have one entry per env")
            self.mean.masked_fill_(m[None, :, None, None], 0.0)


class MPPIPlanner(_SamplingPlanner):
    """Model-predictive path integral control of a continuous-action env (a discrete action mode raises ValueError).

    horizon K >= 1 steps, candidates 1 <= C <= 2^17 per env, exploration `sigma` >= 0 (one value for every step, agent and
    component), temperature `lam` > 0, discount `gamma` in [0, 1], `clip` > 0: candidates are clamped to [-clip, clip]
    (clip <= 0: no clamp).  `sigma`, `lam`, `clip` and `gamma` are plain attributes, read (and checked) at every call.
    `noise_offset` is the planner's OWN counter: step k of a call draws at noise_offset + k, and `plan()` advances it by K, so
    that a plan made one env step later never re-draws the previous plan's noise shifted by one.  It is not the env's RNG
    offset: planning leaves the env's RNG, like everything else of the env, where it was.

    The planner owns `mean` [K, B, N, 2] (zeros at first) and a second buffer the update writes into; `plan()` swaps them.
    """

    _WHO = "MPPIPlanner"

    def __init__(self, env, horizon, candidates, sigma, lam, gamma=1.0, clip=1.0, noise_offset=0):
        self._setup(env, horizon, candidates, noise_offset)
        self.sigma, self.lam, self.gamma, self.clip = sigma, lam, gamma, clip
        self._scalars()
        self.mean, self._spare = self._plan_buffer(), self._plan_buffer()
        self._launches, self._out = {}, None               # the fused route's bound launches and their result buffers

    def _scalars(self):
        """(sigma, lam, gamma, clip) as they are now, checked."""
        return (_real("sigma", self.sigma, lambda v: v >= 0.0), _real("lam", self.lam, lambda v: v > 0.0),
                _real("gamma", self.gamma, lambda v: 0.0 <= v <= 1.0), _real("clip", self.clip, lambda v: True))

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
        """(launch, out) of the fused scoring launch reading the current `mean` (`_binding`)."""
        sc, w, C = self.env.scenario, self.env.world, self.num_candidates
        mean = self.mean
        return self._binding((mean,), gamma, lambda out: sc.bind_rollout_returns_sampled(w, mean, C, out, gamma))

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


class CEMPlanner(_SamplingPlanner):
    """Cross-entropy-method control of a continuous-action env (a discrete action mode raises ValueError): every control
    step `iterations` rounds of "draw C candidates around (mean, std), score them, refit mean and std to the best `elites`
    of each (env, agent)" - PETS' and PlaNet's planner.

    horizon K >= 1, candidates 1 <= C <= 2^17, 1 <= elites <= C, the initial `sigma` >= 0, iterations >= 1, the refit's
    smoothing `alpha` in (0, 1] (new = (1 - alpha) old + alpha fitted), a floor `sigma_min` >= 0 under the refit std,
    `gamma` in [0, 1], `clip` as for `MPPIPlanner`.  All seven are plain attributes, read (and checked) at every call.
    Every iteration draws at its own offset: iteration j of a `plan()` at noise_offset + j K, and `plan()` advances
    `noise_offset` by K iterations, so that no number is drawn twice.  The elites are the E largest returns of a row in the
    order of `fg_plan_cem_update` (ties: the lower candidate first); the selection is exact.

    The planner owns `mean` and `std` [K, B, N, 2] and a spare of each the update writes into.  CEM-MPC restarts its variance
    every control step: `plan()` first fills `std` with `sigma`; only the mean is warm-started."""
    _WHO = "CEMPlanner"

    def __init__(self, env, horizon, candidates, elites, sigma, iterations=3, alpha=1.0, sigma_min=0.0, gamma=1.0, clip=1.0,
                 noise_offset=0):
        self._setup(env, horizon, candidates, noise_offset)
        self.elites, self.sigma, self.iterations, self.alpha, self.sigma_min = elites, sigma, iterations, alpha, sigma_min
        self.gamma, self.clip = gamma, clip
        sigma = self._scalars()[1]
        self.mean, self._spare = self._plan_buffer(), self._plan_buffer()
        self.std, self._std_spare = self._plan_buffer().fill_(sigma), self._plan_buffer()
        self._launches, self._out, self._elite_idx = {}, None, None

    def _scalars(self):
        """(elites, sigma, iterations, alpha, sigma_min, gamma, clip) as they are now, checked."""
        for name, v, hi in (("elites", self.elites, self.num_candidates), ("iterations", self.iterations, None)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1 or (hi and v > hi):
                raise ValueError("CEMPlanner: bad %s %r" % (name, v))
        real = lambda name, ok: _real(name, getattr(self, name), ok, "CEMPlanner")
        return (int(self.elites), real("sigma", lambda v: v >= 0.0), int(self.iterations),
                real("alpha", lambda v: 0.0 < v <= 1.0), real("sigma_min", lambda v: v >= 0.0),
                real("gamma", lambda v: 0.0 <= v <= 1.0), real("clip", lambda v: True))

    def candidates(self, noise_offset=None):
        """The [C, K, B, N, 2] candidates around the current `mean` and `std` at `noise_offset` (None: the planner's), as
        `fg_plan_candidates_std` writes them: what the fused route draws without storing.  Before the first `plan()` `std` is
        `sigma` everywhere, afterwards what the last refit left (`plan()` starts from `sigma` again).  A fresh tensor."""
        clip = self._scalars()[6]
        B, N, K, C = self._dims()
        off = self.noise_offset if noise_offset is None else int(noise_offset)
        dev = self.env.world.device
        out = torch.empty((C, K, B, N, 2), dtype=torch.float32, device=dev)
        _native.check(_native.load().fg_plan_candidates_std(self._params(), B, N, K, C, off & _MASK64, clip, self.mean.data_ptr(),
                                                            self.std.data_ptr(), out.data_ptr(), _native.current_stream(dev)))
        return out

    def _score(self, off, gamma, clip):
        """(returns [C, B, N] as `rollout_returns` chooses them, info) of the candidates around (mean, std) at offset `off`."""
        env = self.env
        if self.path() != "fused":
            return env.rollout_returns(self.candidates(off), gamma)
        sc, w, C = env.scenario, env.world, self.num_candidates
        mean, std = self.mean, self.std
        launch, out = self._binding((mean, std), None, lambda o: sc.bind_rollout_returns_sampled_std(w, mean, std, C, o))
        launch(off, gamma, clip)
        return (out["ret"] if env.shared_reward else out["indiv"]), {"individual_return": out["indiv"], "steps": out["steps"]}

    def _update(self, off, clip, elites, alpha, sigma_min, returns, shift):
        """`fg_plan_cem_update` from (mean, std) into the spare buffers: (the action [B, N, 2] of step 0, the elites' indices
        [E, B, N] int32)."""
        B, N, K, C = self._dims()
        dev = self.env.world.device
        ret = returns if returns.is_contiguous() else returns.contiguous()
        action = torch.empty((B, N, 2), dtype=torch.float32, device=dev)
        if self._elite_idx is None or self._elite_idx.shape[0] != elites:
            self._elite_idx = torch.empty((elites, B, N), dtype=torch.int32, device=dev)
        _native.check(_native.load().fg_plan_cem_update(
            self._params(), B, N, K, C, elites, off, clip, alpha, sigma_min, ret.data_ptr(), self.mean.data_ptr(),
            self.std.data_ptr(), self._spare.data_ptr(), self._std_spare.data_ptr(), action.data_ptr(),
            self._elite_idx.data_ptr(), 1 if shift else 0, _native.current_stream(dev)))
        return action, self._elite_idx

    def plan(self, shift=True):
        """One control step: `std` = `sigma`, then `iterations` rounds of scoring the C candidates around (mean, std) from the
        env's current state and refitting both to each row's `elites` best.  Every round but the last keeps the plan aligned
        (shift 0); with `shift` the last one moves it one step on, its last step repeated: the receding horizon.  Returns
        (action [B, N, 2] - step 0 of the last refit mean -, info = {'returns', 'individual_return' [C, B, N] and 'steps' [B]
        of the last iteration, 'std' [K, B, N, 2] after it, 'elites' [E, B, N] int32: its elites' candidate indices in
        ascending order, 'noise_offset': the first offset this call drew at}).  Advances `noise_offset` by K iterations.  The
        env is left exactly as `rollout_returns` leaves it.  The tensors in `info` are the planner's own buffers: the next
        `plan()` overwrites them - clone what must outlive it."""
        elites, sigma, iterations, alpha, sigma_min, gamma, clip = self._scalars()
        first = self.noise_offset & _MASK64
        self.std.fill_(sigma)
        for j in range(iterations):
            off = (first + j * self.horizon) & _MASK64
            returns, info = self._score(off, gamma, clip)
            action, idx = self._update(off, clip, elites, alpha, sigma_min, returns, bool(shift) and j == iterations - 1)
            self.mean, self._spare = self._spare, self.mean
            self.std, self._std_spare = self._std_spare, self.std
        self.noise_offset = (first + iterations * self.horizon) & _MASK64
        return action, {"returns": returns, "individual_return": info["individual_return"], "steps": info["steps"],
                        "std": self.std, "elites": idx, "noise_offset": first}
