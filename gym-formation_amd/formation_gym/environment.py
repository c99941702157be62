"""MultiAgentEnv: the env shell of reference formation_gym/environment.py
(:11-236), driving B environments per call on one MI355X.

Drop-in surface kept: constructor signature, `seed`, `reset`, `step`,
`action_space[]`, `observation_space[]`, `share_observation_space[]`,
`num_agents`, `agents`, `world`, `world_length`, `current_step`, `num_envs`,
`shared_reward`.

Two calling conventions for `step`:
  * reference style - `action_n` is a list of N arrays of shape (2,) (num_envs
    must be 1): returns `(obs_n, reward_n, done_n, info_n)` exactly shaped like
    the reference (lists of float64 arrays / [float] / bool / dict) and, like the
    reference (environment.py:216-221), scales the caller's arrays in place and
    rejects plain Python lists;
  * batched - `action_n` is a float32 tensor [B, N, 2] on the device: returns
    device tensors obs [B,N,6N], reward [B,N,1], done [B,N] (bool) and
    info = {'individual_reward': [B,N]}.  These are views of buffers that the
    next `step` overwrites.
Either way ONE fused HIP launch does `_set_action` (x N), `world.step()` and the
N observation / 2N reward / N done callbacks of environment.py:113-142.
"""
import numbers

import numpy as np
import torch

from . import _native, actor_rollout, placement, spaces

cam_range = 2


class MultiAgentEnv(object):
    metadata = {'render.modes': ['human', 'rgb_array']}

    def __init__(self, world, reset_callback=None, reward_callback=None,
                 observation_callback=None, info_callback=None,
                 done_callback=None, post_step_callback=None,
                 shared_viewer=True, discrete_action=False):
        self.world = world
        self.world_length = self.world.world_length
        self.current_step = 0
        self.agents = self.world.policy_agents
        self.num_agents = len(world.policy_agents)
        self.reset_callback = reset_callback
        self.reward_callback = reward_callback
        self.observation_callback = observation_callback
        self.info_callback = info_callback
        self.done_callback = done_callback
        self.post_step_callback = post_step_callback
        self.num_envs = world.num_envs
        self.scenario = world.scenario
        if self.scenario is None:
            raise ValueError("world.scenario is not set: make_world() must attach the Scenario "
                             "that owns the batched kernels")
        # action modes (environment.py:39-47): make_env never sets them, direct construction may
        self.discrete_action_space = bool(discrete_action)        # 5-vector per agent, u = (a1-a2, a3-a4)
        self.discrete_action_input = False                        # an index 0..4 per agent
        self.force_discrete_action = bool(getattr(world, 'discrete_action', False))   # arg-max one-hot
        self.shared_reward = world.collaborative if hasattr(world, 'collaborative') else False
        self.time = 0
        self.auto_reset = False           # vec-env worker semantics, see vec_env.py
        self._rng_offset = 0

        # spaces (environment.py:55-96)
        self.action_space = []
        self.observation_space = []
        obs_dim = self.scenario.obs_dim(world)
        share_obs_dim = 0
        for agent in self.agents:
            if self.discrete_action_space:                        # :64-65
                u_space = spaces.Discrete(world.dim_p * 2 + 1)
            else:
                u_space = spaces.Box(low=-agent.u_range, high=+agent.u_range, shape=(world.dim_p,), dtype=np.float32)
            if not agent.silent:                                  # :72-84: a Tuple (physical, communication) action space
                c_space = spaces.Discrete(world.dim_c) if self.discrete_action_space else \
                    spaces.Box(low=0.0, high=1.0, shape=(world.dim_c,), dtype=np.float32)
                self.action_space.append(spaces.Tuple([u_space, c_space]))
            else:
                self.action_space.append(u_space)
            share_obs_dim += obs_dim
            self.observation_space.append(spaces.Box(low=-np.inf, high=+np.inf,
                                                     shape=(obs_dim,), dtype=np.float32))
        self.share_observation_space = [spaces.Box(low=-np.inf, high=+np.inf, shape=(share_obs_dim,),
                                                   dtype=np.float32) for _ in range(self.num_agents)]

        B, N = self.num_envs, self.num_agents
        dev = world.device
        f = dict(dtype=torch.float32, device=dev)
        # the four per-step outputs are views of ONE allocation, so that the reference-style API
        # (num_envs == 1: NumPy lists in and out) brings a whole step back in a single device-to-host copy
        n_obs, n_bn = B * N * obs_dim, B * N
        self._flat = torch.zeros(n_obs + 2 * n_bn + (n_bn + 3) // 4, **f)
        self._out = dict(
            obs=self._flat[:n_obs].view(B, N, obs_dim),
            reward=self._flat[n_obs:n_obs + n_bn].view(B, N),
            indiv=self._flat[n_obs + n_bn:n_obs + 2 * n_bn].view(B, N),
            done=self._flat[n_obs + 2 * n_bn:].view(torch.uint8)[:n_bn].view(B, N),
        )
        self._act = torch.zeros((B, N, 2), **f)
        self._host = self._act_host = None
        if B == 1 and torch.device(dev).type == "cuda":       # pinned mirrors for the single-env list API
            self._host = torch.empty(self._flat.shape, dtype=torch.float32).pin_memory()
            self._act_host = torch.zeros((1, N, 2), dtype=torch.float32).pin_memory()
        self._launchers = {}              # pre-bound step launches, see _bound_step
        self._roll_launchers = {}         # pre-bound K-step launches into caller-owned buffers, see rollout
        self.placement = None             # report of the last buffer placement probe (alloc_rollout_buffers)
        self._auto_out = {}               # (K, obs_every, policy) -> placed output buffers of rollout(out=None), see _default_out
        # rollout(out=None): env-owned, placed, re-used buffers (False: fresh tensors per call)
        self.default_placed = bool(getattr(self.scenario, "DEFAULT_PLACED", True))
        self.shared_viewer = shared_viewer
        self.viewers = [None]

    # ------------------------------------------------------------------ seed
    def seed(self, seed=None):
        """environment.py:106-110 (default seed 1)."""
        self.scenario.seed(seed)

    def enable_assignments(self, on=True):
        """Also emit the landmark-index assignments (nearest ideal point per
        agent, nearest agent per ideal point, Hausdorff witness pairs) each step."""
        self._launchers.clear()           # bound launches hold the old output pointers
        B, N = self.num_envs, self.num_agents
        dev = self.world.device
        if on:
            self._out["near_lm"] = torch.zeros((B, N), dtype=torch.int32, device=dev)
            self._out["near_ag"] = torch.zeros((B, N), dtype=torch.int32, device=dev)
            self._out["hd_idx"] = torch.zeros((B, 4), dtype=torch.int32, device=dev)
        else:
            for k in ("near_lm", "near_ag", "hd_idx"):
                self._out.pop(k, None)

    # ------------------------------------------------------------------ step
    def step(self, action_n):
        self.current_step += 1
        self.agents = self.world.policy_agents
        if self.world.any_frozen_silent():
            # environment.py:191-236: `_set_action` consumes the action only `if agent.movable` (or as the communication of
            # a non-silent agent) and then asserts that nothing is left - a silent immovable agent trips that assertion
            # (fixture hd_n6_immovable records it).  Such agents are driven through the World API: world.step().
            raise AssertionError
        if self.world.any_non_silent():
            # The reference cannot step non-silent (movable) agents either: `_set_action` consumes the whole action for
            # the physical part and then indexes the exhausted list for the communication part (environment.py:216-231;
            # fixture hd_n5_comm records the IndexError).  Non-silent agents are driven through the World API instead:
            # agent.action.u / agent.action.c, world.step(), scenario.observation / reward (core.py:206-225, 279-286).
            raise IndexError("list index out of range")
        batched = torch.is_tensor(action_n)
        mode = self._action_mode()
        if mode:
            act = self._decode_actions(action_n, mode, batched)
        elif batched:
            act = action_n
            if act.shape != self._act.shape:
                raise ValueError("batched action must have shape %s, got %s"
                                 % (tuple(self._act.shape), tuple(act.shape)))
            if act.dtype != torch.float32 or act.device != self._act.device or not act.is_contiguous():
                self._act.copy_(act)
                act = self._act
        else:
            act = self._stage_reference_actions(action_n)
        off = self._launch_rng_offset()
        if not self._bound_step(act, off):
            self.scenario.step_batch(self.world, act, self._out, auto_reset=self.auto_reset, rng_offset=off)
        self._advance_rng(1)
        self.world.world_step += 1
        if self.post_step_callback is not None:
            self.post_step_callback(self.world)
        if batched:
            return self._batched_result()
        return self._reference_result()

    def rollout(self, action_seq, out=None, obs_every=1, obs_dtype=None):
        """K consecutive `step` calls in ONE launch (`fg_rollout_hd`): for policies that hand over a
        whole action sequence (open-loop / pre-staged random policies; for model-predictive candidates - the returns of C
        sequences from the SAME state, the env left where it was - see `rollout_returns`).
        `action_seq` is a [K, B, N, 2] tensor of raw continuous actions.  Results are bit-identical to
        K calls of `step` (device auto-reset included, when `self.auto_reset` is set) and come back
        stacked along a leading step axis:
            obs [K // obs_every, B, N, D]  (every obs_every-th step; obs_every = 1: every step)
            reward [K, B, N, 1], done [K, B, N] bool, info {'individual_reward': [K, B, N]}
        `out` may hold pre-allocated buffers (keys obs, reward, indiv, done with those shapes, done as
        uint8), so that a training loop re-uses them.  out=None (the default): the env's own buffers for this (K,
        obs_every), made on first use with the observation buffer PLACED (`alloc_rollout_buffers`: one probe per shape,
        0.2-0.4 s and transiently up to 6 x the buffer of device memory - the implicit path never escalates to larger
        arenas) and re-used by every later call.  LIKE `step`, THE RESULTS ARE VIEWS OF ENV-OWNED BUFFERS THAT THE NEXT
        `rollout` OF THE SAME SHAPE OVERWRITES: `traj.append(env.rollout(a))` aliases - clone what must outlive the next
        call, or pass out=False (fresh, ordinary tensors on every call) or your own `out`.  The four most recently used
        (K, obs_every, policy) shapes keep their buffers; `env.default_placed = False` makes out=None mean out=False.
        `obs_dtype` = torch.float16 or torch.bfloat16: the returned obs has that dtype and holds, bit for bit, what
        `.to(obs_dtype)` of the fp32 launch's observations holds (round to nearest even); everything else, the state left
        behind and the RNG counter are the fp32 launch's.  `obs_path(obs_dtype)` tells how: 'fused' - the launch itself stores
        16-bit units (`fg_rollout_hd_obs16`: half the observation bytes, no second pass) - or 'cast' - the fp32 launch into
        the env's usual buffers, then a cast.  With `obs_dtype`, `out` is a caller's dict whose out["obs"] is a CONTIGUOUS
        tensor of that dtype (a padded env pitch raises ValueError), and out=None means out=False: fresh, ordinary tensors per
        call - the placement probe is not extended to 16-bit buffers."""
        fmt = _native.obs_format(obs_dtype)
        if fmt and (len(action_seq) < 2 or self.obs_path(obs_dtype) == "cast"):
            return self._rollout_cast(obs_dtype, out, len(action_seq), int(obs_every), False,
                                      lambda o: self.rollout(action_seq, o, obs_every))
        out, first = self._rollout_into(action_seq, out, obs_every, obs_dtype)
        return self._rollout_result(out, rew=first)

    def _rollout_into(self, action_seq, out, obs_every, obs_dtype=None):
        """`rollout` up to its result: (the `out` the K steps were written to - obs, reward (shared), indiv, done -, the reward
        `rollout` returns where it is not out's: a Scenario file's first_reward of the host-paced loop, else None)."""
        roll = getattr(self.scenario, "rollout_batch", None)
        if roll is None or self.post_step_callback is not None:
            # no multi-step launch (a reference-style Scenario file: its callbacks run on the host), or a post_step_callback
            # (environment.py:140-141: a host function after every step): K `step` calls behind the same interface
            return self._rollout_by_steps(action_seq, out, obs_every)
        mode = self._action_mode()
        if mode:
            # the discrete action modes of _set_action (environment.py:194-215): the whole sequence is decoded to raw u in
            # ONE launch (`fg_decode_actions` over K B N entries), then the K steps run as for continuous actions
            act = self._decode_action_seq(action_seq, mode)
        else:
            if not torch.is_tensor(action_seq) or action_seq.dim() != 4 or tuple(action_seq.shape[1:]) != tuple(self._act.shape):
                raise ValueError("action_seq must be a tensor of shape [K, %d, %d, 2]" % tuple(self._act.shape[:2]))
            act = action_seq
            if act.dtype != torch.float32 or act.device != self._act.device or not act.is_contiguous():
                act = act.to(device=self._act.device, dtype=torch.float32).contiguous()
        K, obs_every = self._check_steps(act.shape[0], obs_every)
        want = self._rollout_shapes(K, obs_every)
        out, own_buffers = self._rollout_out(want, out, K, obs_every, False, obs_dtype)
        self._run_rollout(("roll", act.data_ptr(), K), want, out, own_buffers, K, obs_every, obs_dtype,
                          getattr(self.scenario, "bind_rollout", None), roll, (act,))
        return out, None

    # ---- returns of candidate action sequences from the current state ------------------------------------------------------
    RETURNS_FUSED_N = (3, 4, 8, 9, 16, 25, 27, 32)        # the agent counts returns_kernel is built for (fg_returns_kernel.hpp)

    def returns_path(self):
        """'fused' when `rollout_returns` runs as ONE launch that leaves the env untouched (`fg_rollout_hd_returns`), 'replay'
        when it runs the same contract through the existing launches (snapshot, one `rollout` per candidate, restore).
        'fused' needs a scenario with `bind_rollout_returns` (formation_hd_env), one of its agent counts (3, 4, 8, 9, 16, 25,
        27, 32), no World options (walls, u_noise, max_speed, accel, per-agent properties, communication: the predicate of
        `_resolve_actor`), silent agents, no scripted agents and no post_step_callback.  Decided without touching the device."""
        sc = self.scenario
        if getattr(sc, "bind_rollout_returns", None) is None or self.post_step_callback is not None \
                or getattr(self, "_returns_replay_only", False):      # (the private switch: tests hold the replay to the fused bits)
            return "replay"
        if self.num_agents not in self.RETURNS_FUSED_N or self.world.any_non_silent():
            return "replay"
        try:
            p = sc.params(self.world)
        except NotImplementedError:                        # scripted agents: only the World API drives them
            return "replay"
        if p.num_walls > 0 or p.u_noise > 0 or p.max_speed > 0 or p.accel > 0 or p.agent_props or p.comm_state:
            return "replay"
        return "fused"

    def _check_returns_actions(self, action_seqs):
        """`rollout_returns`' candidates: [C, K] in front of `rollout`'s per-step shape in the env's action mode, C >= 1, K >= 1.
        Returns (mode, the dtype the launches read)."""
        B, N = self.num_envs, self.num_agents
        mode = self._action_mode()
        tail, dtype = {0: ((B, N, 2), torch.float32),
                       _native.FG_ACT_ONEHOT5: ((B, N, 5), torch.float32),
                       _native.FG_ACT_INDEX: ((B, N), torch.int32),
                       _native.FG_ACT_ARGMAX: ((B, N, 2), torch.float32)}[mode]
        if not torch.is_tensor(action_seqs) or action_seqs.dim() != len(tail) + 2 or tuple(action_seqs.shape[2:]) != tail \
                or action_seqs.shape[0] < 1 or action_seqs.shape[1] < 1:
            raise ValueError("action_seqs must be a tensor of shape [C, K%s] with C >= 1 and K >= 1"
                             % "".join(", %d" % d for d in tail))
        return mode, dtype

    def _returns_actions(self, action_seqs):
        """The checked candidates as raw u [C, K, B, N, 2], fp32 contiguous on the env's device.  In a discrete action mode they
        are decoded in ONE `fg_decode_actions` launch over all C K B N entries (force_discrete_action: the caller's array is
        rewritten as the one-hot, as `rollout` does)."""
        mode, dtype = self._check_returns_actions(action_seqs)
        B, N = self.num_envs, self.num_agents
        dev = self._act.device
        src = action_seqs
        if src.dtype != dtype or src.device != dev or not src.is_contiguous():
            src = src.to(device=dev, dtype=dtype).contiguous()
        if not mode:
            return src
        C, K = int(src.shape[0]), int(src.shape[1])
        u = torch.empty((C, K, B, N, 2), dtype=torch.float32, device=dev)
        _native.check(_native.load().fg_decode_actions(mode, C * K * B * N, src.data_ptr(), u.data_ptr(),
                                                       _native.current_stream(dev)))
        if mode == _native.FG_ACT_ARGMAX and src is not action_seqs:
            action_seqs.copy_(src)                     # the reference overwrites the caller's array (:213-215)
        return u

    def rollout_returns(self, action_seqs, gamma=1.0):
        """Score C candidate action sequences from the CURRENT state and leave the env where it was: what a planner (random
        shooting, CEM, MPPI) or a trainer that weighs alternatives asks of the simulator.  `action_seqs` is [C, K, B, N, 2]
        (each `action_seqs[c]` a valid argument of `rollout`; in the discrete action modes `rollout`'s per-step shape behind
        the leading C), converted to fp32 contiguous on the env's device like `rollout`'s.  For every candidate c and env b
        the K steps are exactly those `rollout(action_seqs[c])` runs with `auto_reset` off, from env b's current state; with
        their shared rewards, individual rewards and done flags r_k,
            d_0 = 1, d_{k+1} = d_k * gamma;   R_k = R_{k-1} + d_k * r_k   for k < steps[b]          (R_{-1} = 0)
        in fp32, every product and every sum rounded on its own.  A step counts while no earlier step of this call has set the
        done flag: the step that sets it counts, nothing after it does, and no reset is drawn -
        steps[b] = min(K, max(1, world_length - step_count[b])), the same for every candidate.
        Returns (returns, info): returns [C, B, N] fp32, the recurrence on the shared reward when `shared_reward`, else on the
        individual one (the choice `rollout` makes); info = {'individual_return': [C, B, N] fp32, 'steps': [B] int32}.  Fresh
        tensors that alias nothing.
        NOTHING OF THE ENV CHANGES: state, step counters, ideal shape and velocity, the RNG offset (or device counter),
        `current_step`, `world.world_step`, `auto_reset`, the env-owned rollout buffers and their zero-primed registration.
        `returns_path()` tells how.  'fused': ONE launch (`fg_rollout_hd_returns`) that reads the state and writes only the
        results - a few floats per (candidate, env), no observation, no per-step reward.  'replay': `_snapshot()`, then per
        candidate `_restore` and `rollout(action_seqs[c], out=False, obs_every=K)` with `auto_reset` off, the recurrence in
        torch fp32 ops on its outputs, and in a `finally` `_restore` and the old `auto_reset` - every scenario, agent count and
        World option, and on a fused shape the fused launch's bits.  With motor noise (`u_noise`) every candidate starts from the same RNG offset:
        the candidates are compared under common random numbers.
        ValueError: a wrong shape, C < 1 or K < 1, a `gamma` that is not a finite number in [0, 1]."""
        if isinstance(gamma, bool) or not isinstance(gamma, numbers.Real) or not (0.0 <= float(gamma) <= 1.0):
            raise ValueError("gamma must be a finite number in [0, 1]")
        gamma = float(gamma)
        if self.returns_path() == "replay":
            return self._returns_by_replay(action_seqs, gamma)
        act = self._returns_actions(action_seqs)
        C, K = int(act.shape[0]), int(act.shape[1])
        B, N = self.num_envs, self.num_agents
        dev = self._act.device
        out = dict(ret=torch.empty((C, B, N), dtype=torch.float32, device=dev),
                   indiv=torch.empty((C, B, N), dtype=torch.float32, device=dev),
                   steps=torch.empty((B,), dtype=torch.int32, device=dev))
        # fresh results per call: nothing to key a cached binding on, so the launch is bound and made at once
        self.scenario.bind_rollout_returns(self.world, act, out, gamma)(0)
        return (out["ret"] if self.shared_reward else out["indiv"]), {"individual_return": out["indiv"], "steps": out["steps"]}

    def _returns_by_replay(self, action_seqs, gamma):
        """`rollout_returns` through the existing launches (see there)."""
        self._check_returns_actions(action_seqs)
        C, K = int(action_seqs.shape[0]), int(action_seqs.shape[1])
        B, N = self.num_envs, self.num_agents
        dev = self._act.device
        ret = torch.empty((C, B, N), dtype=torch.float32, device=dev)
        indiv = torch.empty((C, B, N), dtype=torch.float32, device=dev)
        steps = torch.zeros((B,), dtype=torch.int32, device=dev)
        g = torch.tensor(gamma, dtype=torch.float32, device=dev)
        snap, auto_reset = self._snapshot(), self.auto_reset
        self.auto_reset = False
        try:
            for c in range(C):
                self._restore(snap)
                # `rollout(action_seqs[c], out=False)` up to its out dict, which has the shared reward whatever `shared_reward`
                # says; one observation block, at the last step
                out = self._rollout_into(action_seqs[c], False, K)[0]
                rew, own, done = out["reward"], out["indiv"], out["done"][:, :, 0].to(torch.int32)   # the done flag is the env's
                counts = torch.cumsum(done, 0) - done == 0      # [K, B]: a step counts while no EARLIER step has set the flag
                d = torch.ones((), dtype=torch.float32, device=dev)
                r_sh = torch.zeros((B, N), dtype=torch.float32, device=dev)
                r_own = torch.zeros((B, N), dtype=torch.float32, device=dev)
                for k in range(K):
                    m = counts[k][:, None]
                    r_sh = torch.where(m, r_sh + d * rew[k], r_sh)
                    r_own = torch.where(m, r_own + d * own[k], r_own)
                    d = d * g
                ret[c], indiv[c] = r_sh, r_own
                if c == 0:
                    steps.copy_(counts.sum(0).to(torch.int32))
        finally:
            self._restore(snap)
            self.auto_reset = auto_reset
        return (ret if self.shared_reward else indiv), {"individual_return": indiv, "steps": steps}

    # ---- the one path of the three K-step launches: rollout, rollout_policy, rollout_actor --------------------------------
    @staticmethod
    def _check_steps(K, obs_every):
        """(K, obs_every) as ints: at least one step, and an observation every `obs_every` >= 1 steps."""
        K, obs_every = int(K), int(obs_every)
        if K < 1 or obs_every < 1:
            raise ValueError("need K >= 1 steps and obs_every >= 1")
        return K, obs_every

    def _rollout_shapes(self, K, obs_every, act=False, log_prob=False, rnn_states=None, idx=False):
        """The shapes of a K-step launch's outputs by key of `out`: obs, reward, indiv and done always; `act` (the closed
        loops' actions), `log_prob` (a Gaussian or categorical actor's), `rnn_states` (that shape: the kept hidden states) and
        `idx` (a categorical or Gumbel-softmax actor's indices, int32) on request."""
        B, N = self.num_envs, self.num_agents
        want = dict(obs=(K // obs_every, B, N, self._out["obs"].shape[-1]), reward=(K, B, N), indiv=(K, B, N), done=(K, B, N))
        if act:
            want["act"] = (K, B, N, 2)
        if log_prob:
            want["log_prob"] = (K, B, N)
        if rnn_states is not None:
            want["rnn_states"] = tuple(rnn_states)
        if idx:
            want["idx"] = (K, B, N)
        return want

    def _rollout_out(self, want, out, K, obs_every, policy, obs_dtype=None):
        """(`out` resolved, whether its launch may be cached).  None: the env's placed buffers of this shape (`_default_out`)
        while `default_placed` is set and no 16-bit format is asked for, else as False; the optional tensors (log_prob,
        rnn_states) are kept with them, under the same aliasing rule - another rnn_states shape replaces the kept one.  False:
        fresh tensors per call, never cached.  A caller's dict: itself; one without an optional tensor gets a fresh one in a
        copy, and that call is not cached."""
        placed = out is None and self.default_placed and obs_dtype is None
        if placed:
            out = self._default_out(K, obs_every, policy)
        elif out is None or out is False:
            return {k: self._fresh_out(k, want[k], obs_dtype) for k in want}, False
        own_buffers = True
        for k in ("log_prob", "rnn_states", "idx"):
            if k not in want:
                continue
            if placed and tuple(getattr(out.get(k), "shape", ())) != want[k]:
                out[k] = self._fresh_out(k, want[k])
            elif k not in out:
                out, own_buffers = dict(out, **{k: self._fresh_out(k, want[k])}), False
            elif k == "rnn_states":
                self._state_tensor("out['rnn_states']", out[k], want[k], None)
            elif k == "idx" and (not torch.is_tensor(out[k]) or out[k].dtype != torch.int32):
                raise ValueError("out['idx'] must be an int32 tensor of shape %s" % (want[k],))
        return out, own_buffers

    def _fresh_out(self, k, shape, obs_dtype=None):
        """A new tensor for key `k` of `out`: done as zeroed bytes, idx as int32, obs in `obs_dtype` if given, everything else
        fp32."""
        if k == "done":
            return torch.zeros(shape, dtype=torch.uint8, device=self._act.device)
        if k == "idx":
            return torch.empty(shape, dtype=torch.int32, device=self._act.device)
        return torch.empty(shape, dtype=(obs_dtype or torch.float32) if k == "obs" else torch.float32, device=self._act.device)

    def _run_rollout(self, lead_key, want, out, own_buffers, K, obs_every, obs_dtype, bind, unbound, args, extra=()):
        """One K-step launch into `out`, and the env's bookkeeping after it.  Launches into CALLER-OWNED (or env-owned, placed)
        buffers are bound once per (`lead_key`: what the launch reads besides - actions, weights, states -, buffers, stream,
        constants): a training loop that re-uses its buffers pays one dict lookup and one ctypes call per launch (cf.
        _bound_step).  A binding keeps its tensors alive (their addresses are baked in), so the cache is small - cleared when
        it holds 8 - and skips internally allocated outputs.  `bind(world, *args, out, ...)` is the scenario's `bind_*`
        (None: it has none), `unbound` its launch-at-once twin for what is not cached (None: bind anyway); `extra`: further
        keywords of `bind`.  `out` is checked against `want` when a launch is bound or runs unbound, not on a cache hit."""
        key = None
        if own_buffers and bind is not None and want.keys() <= out.keys():
            key = lead_key + (tuple([out[k].data_ptr() for k in want]), tuple(out["obs"].stride()), obs_every,
                              self.auto_reset, _native.current_stream_fast(self.world.device), self.world.params_signature(),
                              getattr(self.scenario, "_seed", 0), obs_dtype, placement._primed_gen[0])
        launch = self._roll_launchers.get(key) if key is not None else None
        off = self._launch_rng_offset()
        if launch is None:
            for k, shp in want.items():
                if k not in out or tuple(out[k].shape) != shp or not (out[k].is_contiguous() or k == "obs"):
                    raise ValueError("out[%r] must be a contiguous tensor of shape %s" % (k, shp))   # obs: or a padded env pitch
            self._check_obs_dtype(out, obs_dtype)
            kw = dict(extra, obs_every=obs_every, auto_reset=self.auto_reset)
            if obs_dtype is not None:
                kw["obs_format"] = _native.obs_format(obs_dtype)
            if key is not None or unbound is None:
                launch = bind(self.world, *args, out, **kw)
            if key is not None:
                if len(self._roll_launchers) >= 8:
                    self._roll_launchers.clear()
                self._roll_launchers[key] = launch
        if launch is not None:
            launch(off)
            self.scenario._cache = None
        else:
            unbound(self.world, *args, out, rng_offset=off, **kw)
        self._advance_rng(K)
        self.current_step += K
        self.world.world_step += K

    def _rollout_result(self, out, info=(), rew=None):
        """(obs, reward [..., 1], done as bool, info) of a K-step call from its `out`; `info`: the keys besides
        'individual_reward'; `rew`: the per-agent reward where it is not out's (shared: out["reward"], else out["indiv"])."""
        if rew is None:
            rew = out["reward"] if self.shared_reward else out["indiv"]
        info = dict(info, individual_reward=out["indiv"])
        return out["obs"], rew.unsqueeze(-1), out["done"].view(torch.bool), info

    def _rollout_by_steps(self, action_seq, out, obs_every):
        """`rollout` as K calls of `step` (host-paced: one launch - and whatever the scenario / the post_step_callback does on
        the host - per step), results stacked like `rollout`'s, as `_rollout_into` returns them."""
        K, obs_every = self._check_steps(len(action_seq), obs_every)
        dev = self._act.device
        want = self._rollout_shapes(K, obs_every)
        if out is None or out is False:
            out = self._rollout_out(want, False, K, obs_every, False)[0]
        for k, shp in want.items():
            if k not in out or tuple(out[k].shape) != shp:
                raise ValueError("out[%r] must be a tensor of shape %s" % (k, shp))
        first = None if self.shared_reward else torch.empty(want["reward"], dtype=torch.float32, device=dev)
        if torch.is_tensor(out["obs"]) and out["obs"].numel():
            # the observations are COPIED in below, not written by a launch that Scenario.params has seen: whatever the steps
            # put into the communication block lands in this buffer, so it is no longer known to hold zeros there
            placement.drop_primed(out["obs"].data_ptr(), out["obs"].numel() * out["obs"].element_size())
        for k in range(K):
            act = action_seq[k]
            if torch.is_tensor(act) and (act.dtype != torch.float32 or act.device != dev) and not self._action_mode():
                act = act.to(device=dev, dtype=torch.float32)
            o, r, d, info = self.step(act if torch.is_tensor(act) else torch.as_tensor(act, device=dev))
            out["reward"][k].copy_(self._out["reward"]); out["indiv"][k].copy_(self._out["indiv"])
            out["done"][k].copy_(self._out["done"])
            if first is not None:
                first[k].copy_(r[..., 0])
            if (k + 1) % obs_every == 0:
                out["obs"][k // obs_every].copy_(o)
        return out, first                                # not shared: what `step` returned (a Scenario file's first_reward)

    def _step_loop(self, K, obs_every, act_fn, after_step=None):
        """The host-paced closed loop, K x (act = act_fn(obs, k); obs, ... = step(act); after_step(done)), from the env's
        current observation, stacked like a K-step launch's results (fresh tensors; obs every `obs_every`-th step, an empty
        [0, B, N, D] when there is none), the actions taken under info['actions']."""
        res = {k: [] for k in ("obs", "rew", "done", "indiv", "act")}
        obs = self._out["obs"]
        for k in range(K):
            act = act_fn(obs, k)
            res["act"].append(act.clone() if torch.is_tensor(act) else torch.as_tensor(act, device=self._act.device))
            obs, r, d, info = self.step(act)
            if (k + 1) % obs_every == 0:
                res["obs"].append(obs.clone())
            res["rew"].append(r.clone()); res["done"].append(d.clone()); res["indiv"].append(info["individual_reward"].clone())
            if after_step is not None:
                after_step(d)
        return (torch.stack(res["obs"]) if res["obs"] else obs.new_empty((0,) + tuple(obs.shape)), torch.stack(res["rew"]),
                torch.stack(res["done"]), {"individual_reward": torch.stack(res["indiv"]), "actions": torch.stack(res["act"])})

    def rollout_policy(self, K, num_agents_per_layer=3, out=None, obs_every=1, obs_dtype=None):
        """The reference's demo loop (test.py:17-27) for K steps in one call:
            act_n = get_action_BFS(ezpolicy, obs_n, num_agents_per_layer); obs_n, ... = env.step(act_n)
        starting from the current state (`fg_rollout_hd_policy`; ONE launch at 3, 9, 27, 81 or 243 agents with
        3 agents per layer).  Results equal K x (`get_action_BFS` on the last observation, `step`) bit for bit and
        come back like `rollout`'s, with the actions taken under info['actions'] [K, B, N, 2].  `obs_dtype`: as `rollout`'s
        (`obs_path(obs_dtype, policy=True)`; the fused launch is `fg_rollout_hd_policy_obs16`, 3 agents per layer)."""
        roll = getattr(self.scenario, "rollout_policy_batch", None)
        if roll is None:
            raise NotImplementedError("%s has no built-in controller" % type(self.scenario).__name__)
        if self._action_mode():
            raise NotImplementedError("the built-in controller emits raw continuous actions")
        K, obs_every = int(K), int(obs_every)
        fmt = _native.obs_format(obs_dtype)
        if fmt and (K < 2 or int(num_agents_per_layer) != 3 or self.obs_path(obs_dtype, policy=True) == "cast"):
            return self._rollout_cast(obs_dtype, out, K, obs_every, True,
                                      lambda o: self.rollout_policy(K, num_agents_per_layer, o, obs_every))
        if self.post_step_callback is not None:
            # a host function after every step (environment.py:140-141): the demo loop itself, launch by launch
            from .policy_bfs import ezpolicy, get_action_BFS
            K, obs_every = self._check_steps(K, obs_every)
            return self._step_loop(K, obs_every, lambda obs, k: get_action_BFS(ezpolicy, obs, int(num_agents_per_layer)).float())
        K, obs_every = self._check_steps(K, obs_every)
        want = self._rollout_shapes(K, obs_every, act=True)
        out, own_buffers = self._rollout_out(want, out, K, obs_every, True, obs_dtype)
        self._run_rollout(("pol", K, int(num_agents_per_layer)), want, out, own_buffers, K, obs_every, obs_dtype,
                          getattr(self.scenario, "bind_rollout_policy", None), roll, (K, num_agents_per_layer))
        return self._rollout_result(out, {"actions": out["act"]})

    def obs_path(self, obs_dtype, policy=False, actor=None):
        """How `rollout(..., obs_dtype=obs_dtype)` (policy=True: `rollout_policy`, 3 agents per layer; actor=...:
        `rollout_actor` with that actor, 'fused' when the actor resolves to a fused launch - `_resolve_actor` - and the
        library's dry run `fg_describe_actor_obs16_launch` / `fg_describe_actor_cat_obs16_launch` accepts it) produces its 16-bit
        observations: 'fused' - the launch itself stores fp16 / bf16 units (`fg_rollout_hd_obs16`; formation_hd_env at 3, 9
        or 27 agents without World options) - or 'cast' - the fp32 launch runs into the env's usual buffers and the result
        is cast, which is the same bits by definition and works for every scenario, agent count and option.  Decided without
        touching the device: the scenario asks the library (`obs16_supported`, `fg_describe_obs16_launch`); a scenario that
        does not define it (the landmark scenarios, plugin scenarios) runs 'cast', and so does a single step (K = 1)."""
        if not _native.obs_format(obs_dtype):
            raise ValueError("obs_dtype must be torch.float16 or torch.bfloat16")
        sc = self.scenario
        if actor is not None:
            supported = getattr(sc, "actor_obs16_supported", None)
            fused = None if supported is None or self.post_step_callback is not None else self._resolve_actor(actor)
            return "fused" if fused is not None and supported(self.world, 1, fused, self._action_mode()) else "cast"
        supported = getattr(sc, "obs16_supported", None)
        launch = getattr(sc, "rollout_policy_batch" if policy else "rollout_batch", None)
        if supported is None or launch is None or self.post_step_callback is not None:
            return "cast"
        return "fused" if supported(self.world, 2, 3 if policy else 0) else "cast"

    @staticmethod
    def _check_obs_dtype(out, obs_dtype):
        """A launch with `obs_dtype` writes a contiguous out["obs"] of that dtype (obs_dtype None: nothing to check here)."""
        if obs_dtype is None:
            return
        obs = out["obs"]
        if obs.dtype != obs_dtype:
            raise ValueError("out['obs'] must have dtype %s, got %s" % (obs_dtype, obs.dtype))
        if not obs.is_contiguous():
            raise ValueError("a padded env pitch is not supported with obs_dtype: out['obs'] must be contiguous")

    def _rollout_cast(self, obs_dtype, out, K, obs_every, policy, run_fp32):
        """The 'cast' route of `rollout` / `rollout_policy`.  `run_fp32(out)` is the fp32 call.  Without a caller's `out` it
        runs into the env's usual buffers (out=None) and everything comes back as fresh tensors, the observations cast.  With
        one, the launch fills the caller's tensors itself, except that its observations go to the env's usual fp32 buffer
        and are cast into out["obs"] from there."""
        if not isinstance(out, dict):
            obs, rew, done, info = run_fp32(None)
            return obs.to(obs_dtype), rew.clone(), done.clone(), {k: v.clone() for k, v in info.items()}
        if "obs" not in out:
            raise ValueError("out['obs'] must be a contiguous tensor of dtype %s" % obs_dtype)
        self._check_obs_dtype(out, obs_dtype)
        launches = getattr(self.scenario, "rollout_batch", None) is not None and self.post_step_callback is None
        if launches and self.default_placed and K >= 1 and obs_every >= 1:
            obs32 = self._default_out(K, obs_every, policy)["obs"]
        else:
            obs32 = torch.empty(tuple(out["obs"].shape), dtype=torch.float32, device=self._act.device)
        obs, rew, done, info = run_fp32(dict(out, obs=obs32))
        out["obs"].copy_(obs)                              # the cast: round to nearest even, as .to(obs_dtype)
        return out["obs"], rew, done, info

    def actor_path(self, actor):
        """'fused' when `rollout_actor(K, actor)` runs as ONE launch with the actor inside the rollout kernel
        (`fg_rollout_hd_actor`), 'host' when it runs the host-paced loop.  The rules: formation_gym/actor_rollout.py."""
        return "host" if self._resolve_actor(actor) is None else "fused"

    def _resolve_actor(self, actor):
        """`actor_rollout.resolve_actor` with this env's facts: the FusedActor record of the fused launch, or None (host-paced).
        The one resolution `actor_path` and `rollout_actor` share."""
        sc = self.scenario
        fused = getattr(sc, "bind_rollout_actor", None) is not None
        world_options = False
        if fused:
            try:
                p = sc.params(self.world)
            except NotImplementedError:                    # scripted agents: only the World API drives them
                fused = False
            else:
                world_options = bool(p.num_walls > 0 or p.u_noise > 0 or p.max_speed > 0 or p.accel > 0 or p.agent_props
                                     or p.comm_state)
        facts = self._actor_facts() if fused else {}
        if facts is None:                                  # a landmark scenario at a shape without the fused launch
            fused, facts = False, {}
        return actor_rollout.resolve_actor(actor, self.num_agents, self.world.device, fused_scenario=fused,
                                           continuous=not self._action_mode(), action_mode=self._action_mode(),
                                           silent=not self.world.any_non_silent(),
                                           world_options=world_options, callback=self.post_step_callback is not None,
                                           **facts)

    def _actor_facts(self):
        """The scenario's own facts for `actor_rollout.resolve_actor` (input width, admissible agent counts and
        hidden widths, whether a PerAgentActor fuses): {} for formation_hd_env (the functions' defaults), a landmark
        scenario's `actor_fused_rule(world)` - None where its shape has no fused launch."""
        rule = getattr(self.scenario, "actor_fused_rule", None)
        return {} if rule is None else rule(self.world)

    def rollout_actor(self, K, actor, out=None, obs_every=1, obs_dtype=None, noise_state=None, rnn_state=None,
                      rnn_states_every=None):
        """The loop of a learned actor for K steps in one call:
            act_n = actor(obs_n); obs_n, rew_n, done_n, info = env.step(act_n)
        from the current state (step 0 acts on the observation of the current state, step k on the one step k-1 returned -
        after the device auto-reset, when `auto_reset` is set); each agent's observation row (6N floats in formation_hd_env,
        the scenario's observation width in the landmark scenarios) is one row of the actor's input batch.  Results come back
        like `rollout_policy`'s, with the actions taken under info['actions'] [K, B, N, 2],
        and with its aliasing rules for `out`.
        `actor_path(actor)` tells which loop runs.  'fused': ONE launch (`fg_rollout_hd_actor`) with the actor - one
        Sequential(Linear(6N, H), ReLU, Linear(H, H), ReLU, Linear(H, 2) [, Tanh]) shared by all agents, H in {32, 64, 128} -
        evaluated inside the rollout kernel on its parameters in place (an optimizer step between two calls is seen by the
        next one); replaying info['actions'] through `rollout` gives the same bits.  'host': any other callable, the same loop
        in Python under torch.no_grad(), one `step` per action.
        A `GaussianActor(mean, log_std)` explores: step k takes a = mean(o) + exp(log_std) * eps, where eps [B, N, 2] is the
        env's own counter stream at step k's RNG offset (`fg_actor_noise`: seed, global env index, agent - the same draws on
        either path and for a shard as for its slice of the full batch), and info['log_prob'] [K, B, N] holds
        -(eps_0^2 + eps_1^2) / 2 - sum(log_std) - log(2 pi), the log-density of each action.  `out` may carry 'log_prob'.
        It fuses (`fg_rollout_hd_actor_sample`) when its mean would and log_std is a contiguous fp32 [2] tensor on the env's
        device, read in place like the weights.
        A `PerAgentActor([actor_0, ..., actor_{N-1}])` gives agent i its own network, alone or as a GaussianActor's mean; it
        fuses (`fg_rollout_hd_actor_per_agent`) when every member would, with one H and one tanh flag.
        The landmark scenarios (basic_formation_env, formation_hd_partial_env, formation_hd_partial_range_env,
        formation_hd_obs_env) fuse a shared actor, deterministic or Gaussian, at their seven reference shapes with H in
        {32, 64} (`fg_rollout_scenario_actor`); H = 128 and a PerAgentActor run host-paced there.
        The MAPPO trainers' LayerNorm actor (onpolicy's MLPBase) - Sequential([LayerNorm(6N),] Linear(6N, H), ReLU,
        LayerNorm(H), Linear(H, H), ReLU, LayerNorm(H), Linear(H, 2) [, Tanh]), H in {32, 64} - fuses in formation_hd_env
        (`fg_rollout_hd_actor_norm`), alone or as a GaussianActor's mean with the same eps draws and log_prob; its norm
        parameters are read in place like the weights.  Host-paced: H = 128 with norms, any other placement of norms, norm
        parameters in another dtype / non-contiguous / off the device, PerAgentActor members with norms, and a LayerNorm
        actor in the landmark scenarios.
        The MADDPG trainers' BatchNorm actor - Sequential(BatchNorm1d(6N), Linear(6N, H), ReLU, Linear(H, H), ReLU,
        Linear(H, 2) [, Tanh]) in eval mode, H in {32, 64} - fuses in formation_hd_env shared (`fg_rollout_hd_actor_bn`; the
        leading module an `InputBatchNorm`, which takes [B, N, 6N]) or as every member of a PerAgentActor
        (`fg_rollout_hd_actor_bn_per_agent`), alone or as a GaussianActor's mean; the running statistics are read in place,
        and `actor.train()` / `actor.eval()` between calls switch the path.  Host-paced: training mode, a BatchNorm anywhere
        but first, mixed members, H = 128, the landmark scenarios.
        An `OUNoiseActor(actor, theta, sigma, scale, mu, clip)` is the MADDPG trainers' exploration: step k takes
            x = x + theta * (mu - x) + sigma * eps;  a = clamp(actor(o) + scale * x, -clip, clip)
        with eps the GaussianActor's draws (`fg_actor_noise`: the same on either path and for a shard as for its slice of the
        full batch), and x is set to mu where the step's done flag is set, whether or not `auto_reset` is set (the trainers'
        `reset_noise()`).  `noise_state`: a contiguous fp32 [B, N, 2] tensor on the env's device, read as the state step 0
        starts from, updated in place to the state after step K - 1 and returned as info['noise_state']; None: a fresh
        `initial_state` (all mu) per call.  A K-step call equals K one-step calls that pass the state along, bit for bit.  The
        five scalars are read from the module at every call, so `ou.scale = ...` between calls is seen by the next one.  It
        fuses (`fg_rollout_hd_actor_ou`, `fg_rollout_hd_actor_ou_per_agent`; the state on chip for the whole launch) in
        formation_hd_env when its inner actor is the plain or the BatchNorm actor above, shared or a PerAgentActor; a
        LayerNorm inner actor, the landmark scenarios and World options run this loop host-paced, the state stepped by the
        kernels' own device function (`fg_actor_ou_step`).  There is no info['log_prob'] (a GaussianActor's noise stays
        unclipped); `noise_state` with any other actor raises ValueError.
        A `RecurrentActor(base, rnn, norm, head)` (rMAPPO's policy), alone or as a GaussianActor's mean, carries a hidden
        state through the loop:
            a, h = actor(obs, h); obs, rew, done, info = env.step(a); h = h * ~done[..., None]
        (the step's own done flags, whether or not `auto_reset` is set).  `rnn_state`: a contiguous fp32 [B, N, H] tensor on
        the env's device, read as the state step 0 acts with, updated in place to the state after step K - 1 (already masked
        by that step's done flags) and returned as info['rnn_state']; None: a fresh zero tensor per call.  A K-step call
        equals K one-step calls that pass the state along, bit for bit, and so does any other split of K.  It fuses
        (`fg_rollout_hd_actor_gru`, the state on chip for the whole launch) in formation_hd_env when its base with its head
        is the LayerNorm actor above, H in {32, 64}, `rnn` is an nn.GRUCell(H, H) or a single-layer unidirectional
        nn.GRU(H, H) with biases and `norm` a LayerNorm(H); anything else - and the landmark scenarios - runs this loop
        host-paced.  `rnn_state` with an actor that keeps no state raises ValueError.
        `rnn_states_every=S` (an integer >= 1; None: nothing kept, no such key) also keeps the states a recurrent PPO update
        restarts from, on either path: info['rnn_states'] [ceil(K / S), B, N, state_size], fp32 and contiguous on the env's
        device, entry j the state step j * S ACTED WITH (onpolicy's rnn_states[step]) - entry 0 is `rnn_state` as passed in,
        entry j > 0 is already zero where step j * S - 1 ended an episode; S = data_chunk_length keeps only what the recurrent
        generator reads, S > K entry 0 alone.  The fused launch (`fg_rollout_hd_actor_gru_states`) stores them from the chip
        as it goes; nothing else of its results changes, and the entries of a K-step call are those of any split of K.  `out`
        may carry 'rnn_states' of exactly that shape; with out=None the tensor is kept with this shape's env-owned buffers
        like 'log_prob' (replaced when S or the state width changes) under the same aliasing rule - the next out=None call of
        the shape overwrites it - and out=False gives a fresh one per call.  With an actor that keeps no state: ValueError.
        A `CategoricalActor(logits, deterministic=False)` is the MAPPO / rMAPPO trainers' discrete-action policy, for an env
        made with discrete actions (`discrete_action_space`: FG_ACT_ONEHOT5, or `discrete_action_input`: FG_ACT_INDEX): step k
        takes the index drawn from Categorical(logits=logits(o)) by the softmax CDF at the uniform draw `actor_uniform()` of
        step k's RNG offset (the same on either path and for a shard as for its slice of the full batch) - or, with
        `deterministic`, the lowest index of the largest logit - and the env's action mode turns it into the raw action.
        info['actions'] [K, B, N] holds the int32 indices - `env.rollout` takes them back in FG_ACT_INDEX mode and
        `one_hot(actions.long(), 5).float()` in FG_ACT_ONEHOT5 mode, with the same bits - info['u'] [K, B, N, 2] the raw
        actions and info['log_prob'] [K, B, N] the log-probabilities; `out` may carry 'idx' (int32), 'act' (the raw actions)
        and 'log_prob'.  `rnn_state` / `rnn_states_every` as above when `logits` is a RecurrentActor.  It fuses
        (`fg_rollout_hd_actor_cat`) in formation_hd_env on the plain, the LayerNorm and the recurrent form with the head
        Linear(H, 5); per-agent members, a leading BatchNorm, the landmark scenarios and World options run host-paced, the
        pick and the decode by the kernels' own device functions (`fg_actor_categorical`).  Any other actor in a discrete
        action mode, and any actor with `force_discrete_action` (FG_ACT_ARGMAX), raises NotImplementedError; a
        CategoricalActor on an env with continuous actions raises ValueError.
        A `GumbelSoftmaxActor(logits, explore=True)` is the MADDPG trainers' discrete action (maddpg-pytorch's agents), for an
        env made with discrete actions (FG_ACT_ONEHOT5, MADDPG's, or FG_ACT_INDEX): while `explore` is set, step k takes
        argmax_j(logits(o)_j + g_j) - `gumbel_softmax(logits, hard=True)`, whose temperature never changes the index - with g
        [B, N, 5] the draws `actor_gumbel()` of step k's RNG offset, a counter stream of their own (the same on either path and
        for a shard as for its slice of the full batch; the Gaussian, OU and categorical draws keep their bits); otherwise
        `onehot_from_logits`, the lowest index of the largest logit.  `explore` is read at every call.  info['actions']
        [K, B, N] holds the int32 indices (replayable through `rollout` as a CategoricalActor's are), info['u'] [K, B, N, 2] the
        raw actions; there is no info['log_prob'].  `out` may carry 'idx' and 'act'.  It fuses (`fg_rollout_hd_actor_gumbel`,
        `fg_rollout_hd_actor_gumbel_per_agent`) in formation_hd_env when `logits` is the plain or the eval-mode BatchNorm body,
        shared or every member of a PerAgentActor, with the head Linear(H, 5) and no Tanh; a LayerNorm or recurrent body, H =
        128 behind a BatchNorm, mixed members, the landmark scenarios and World options run host-paced, the draws, the pick and
        the decode by the kernels' own device functions (`fg_actor_gumbel`, `fg_actor_gumbel_pick`).  FG_ACT_ARGMAX raises
        NotImplementedError, an env with continuous actions ValueError.  The soft (temperature) sample and epsilon-greedy
        are not built; with `obs_dtype` the observations are cast.
        `obs_dtype` = torch.float16 or torch.bfloat16: as `rollout`'s - the returned obs has that dtype and holds, bit for bit,
        `.to(obs_dtype)` of what the same call without it returns; everything else (actions, log-probs, rewards, done flags,
        the states, the state left behind, the RNG counter) is that call's.  `obs_path(obs_dtype, actor=actor)` tells how:
        'fused' - the actor launch itself stores 16-bit units (`fg_rollout_hd_actor_obs16`, `fg_rollout_hd_actor_cat_obs16`:
        a GaussianActor or CategoricalActor on the plain, the LayerNorm or the recurrent form in formation_hd_env at 3, 9 or
        27 agents, H in {32, 64}, no World options, any K >= 1 and obs_every) - or 'cast' - everything else: the deterministic,
        OU, BatchNorm and per-agent actors, H = 128, the other agent counts, host-paced actors, the landmark scenarios; the
        fp32 call runs, fused or host-paced as without `obs_dtype`, and its observations are cast.  `out` follows `rollout`'s
        rules with `obs_dtype`: a caller's dict with a CONTIGUOUS out["obs"] of that dtype, else fresh tensors per call.
        `FormationVecEnv.rollout_actor` and placed 16-bit buffers are not part of it."""
        fmt = _native.obs_format(obs_dtype)
        mode = self._action_mode()
        cat = actor if isinstance(actor, actor_rollout.CategoricalActor) else None
        gumbel = actor if isinstance(actor, actor_rollout.GumbelSoftmaxActor) else None
        if mode and ((cat is None and gumbel is None) or mode == _native.FG_ACT_ARGMAX):
            raise NotImplementedError("rollout_actor applies the actor's outputs as raw continuous actions")
        if (cat is not None or gumbel is not None) and not mode:
            raise ValueError("a %s needs an env with discrete actions (discrete_action_space or discrete_action_input)"
                             % type(actor).__name__)
        picks = cat is not None or gumbel is not None      # the actor gives an index, which the env's mode decodes
        K, obs_every = self._check_steps(K, obs_every)
        B, N = self.num_envs, self.num_agents
        recurrent = actor_rollout.recurrent_mean(actor)
        if recurrent is None and rnn_state is not None:
            raise ValueError("rnn_state given, but the actor is not a RecurrentActor (nor a GaussianActor with one as its mean)")
        if recurrent is None and rnn_states_every is not None:
            raise ValueError("rnn_states_every given, but the actor is not a RecurrentActor (nor a GaussianActor with one as its "
                             "mean)")
        ou = actor if isinstance(actor, actor_rollout.OUNoiseActor) else None
        if ou is None and noise_state is not None:
            raise ValueError("noise_state given, but the actor is not an OUNoiseActor")
        if ou is not None:                                 # None: a fresh `initial_state`
            noise_state = self._state_tensor("noise_state", noise_state, (B, N, 2),
                                             lambda: ou.initial_state(B, N, device=self.world.device))
        S = None
        if rnn_states_every is not None:
            if isinstance(rnn_states_every, bool) or not isinstance(rnn_states_every, numbers.Integral) or rnn_states_every < 1:
                raise ValueError("rnn_states_every must be an integer >= 1 (or None)")
            S = int(rnn_states_every)
        if recurrent is not None:                          # None: fresh zeros
            shape = (B, N, recurrent.state_size)
            rnn_state = self._state_tensor("rnn_state", rnn_state, shape,
                                           lambda: torch.zeros(shape, dtype=torch.float32, device=self.world.device))
        states_shape = None if S is None else ((K + S - 1) // S,) + tuple(rnn_state.shape)
        if fmt and self.obs_path(obs_dtype, actor=actor) == "cast":
            res = self._rollout_cast(obs_dtype, out, K, obs_every, True,
                                     lambda o: self.rollout_actor(K, actor, o, obs_every, noise_state=noise_state, rnn_state=rnn_state,
                                                                  rnn_states_every=rnn_states_every))
            for key, t in (("rnn_state", rnn_state), ("noise_state", noise_state)):
                if key in res[3]:
                    res[3][key] = t                        # the states come back as updated in place, not as copies
            return res
        fused = self._resolve_actor(actor)
        if fused is None:
            if S is not None and isinstance(out, dict) and "rnn_states" in out:
                self._state_tensor("out['rnn_states']", out["rnn_states"], states_shape, None)
            res = self._rollout_actor_by_steps(K, actor, obs_every, rnn_state, S, noise_state)
            if picks and isinstance(out, dict):
                for key, src in (("idx", "actions"), ("act", "u")) + ((("log_prob", "log_prob"),) if cat is not None else ()):
                    if key in out:
                        res[3][src] = out[key].copy_(res[3][src])
            if S is not None and isinstance(out, dict) and "rnn_states" in out:
                res[3]["rnn_states"] = out["rnn_states"].copy_(res[3]["rnn_states"])
            return res
        want = self._rollout_shapes(K, obs_every, act=True, log_prob=fused.log_std is not None or cat is not None,
                                    rnn_states=states_shape, idx=picks)
        out, own_buffers = self._rollout_out(want, out, K, obs_every, True, obs_dtype)
        # what the launch reads in place besides `out`, by name for the binder and by address for the key: the binding holds
        # the parameter tensors' addresses, so it keys on them (`binding_key`) and keeps them alive - a parameter re-allocated
        # (not updated in place) binds anew
        state = {} if fused.gru is None else {"rnn_state": rnn_state}
        if fused.ou is not None:
            state["noise_state"] = noise_state
        extra = state if S is None else dict(state, rnn_states_every=S)
        if picks:
            extra = dict(extra, act_mode=mode)
        lead = ("actor", K, fused.binding_key(), _native.ptr(rnn_state), S, _native.ptr(noise_state))
        self._run_rollout(lead if not picks else lead + (mode,), want, out,    # the categorical / Gumbel launch bakes the mode in
                          own_buffers, K, obs_every, obs_dtype, self.scenario.bind_rollout_actor, None, (K, fused), extra)
        info = dict(state, actions=out["act"])             # the states come back as updated in place
        if picks:
            info.update(actions=out["idx"], u=out["act"])
        if "log_prob" in want:
            info["log_prob"] = out["log_prob"]
        if S is not None:
            info["rnn_states"] = out["rnn_states"]
        return self._rollout_result(out, info)

    def _state_tensor(self, name, t, shape, fresh):
        """A state tensor a launch reads and writes in place - `rnn_state`, `noise_state`, out['rnn_states'] - as the caller
        passed it: `fresh()` for None (where there is a `fresh`), else `t` itself, checked to be contiguous fp32 of `shape` on
        the env's device."""
        if t is None and fresh is not None:
            return fresh()
        shape, dev = tuple(shape), self.world.device
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() \
                or not actor_rollout._on_device(t, dev):
            raise ValueError("%s must be a contiguous float32 tensor of shape %s on %s" % (name, shape, dev))
        return t

    def _ou_step(self, ou, eps, x):
        """x <- x + theta * (mu - x) + sigma * eps in place (`fg_actor_ou_step`: the fused kernels' device function)."""
        _native.check(_native.load().fg_actor_ou_step(_native.actor_ou(ou), x.numel() // 2, eps.data_ptr(), x.data_ptr(),
                                                      _native.current_stream(self.world.device)))
        return x

    def actor_noise(self, out=None):
        """The exploration noise eps [B, N, 2] that a GaussianActor's next step draws (`fg_actor_noise` at the offset of the
        next launch): what `rollout_actor` adds, scaled by exp(log_std), to the mean action of that step."""
        B, N = self.num_envs, self.num_agents
        if out is None:
            out = torch.empty((B, N, 2), dtype=torch.float32, device=self.world.device)
        sc = self.scenario
        p = self.world.native_params(seed=getattr(sc, "_seed", 0), rng_offset=self._launch_rng_offset(), scripted_ok=True)
        p.env_index_base = int(getattr(sc, "env_base", 0))
        _native.check(_native.load().fg_actor_noise(p, B, N, out.data_ptr(), _native.current_stream(self.world.device)))
        return out

    def actor_uniform(self, out=None):
        """The uniform draws u [B, N] in [0, 1) that a CategoricalActor's next step samples with (`fg_actor_uniform` at the
        offset of the next launch): word 2 of the Philox block whose words 0 and 1 give `actor_noise()`."""
        B, N = self.num_envs, self.num_agents
        if out is None:
            out = torch.empty((B, N), dtype=torch.float32, device=self.world.device)
        sc = self.scenario
        p = self.world.native_params(seed=getattr(sc, "_seed", 0), rng_offset=self._launch_rng_offset(), scripted_ok=True)
        p.env_index_base = int(getattr(sc, "env_base", 0))
        _native.check(_native.load().fg_actor_uniform(p, B, N, out.data_ptr(), _native.current_stream(self.world.device)))
        return out

    def actor_gumbel(self, out=None):
        """The Gumbel draws g [B, N, 5] that a GumbelSoftmaxActor's next step explores with (`fg_actor_gumbel` at the offset of
        the next launch): -log(-log(u)) of five uniforms in (0, 1) per (env, agent) from a Philox stream of their own, so
        `actor_noise()` and `actor_uniform()` keep their bits."""
        B, N = self.num_envs, self.num_agents
        if out is None:
            out = torch.empty((B, N, actor_rollout.CAT_ACTIONS), dtype=torch.float32, device=self.world.device)
        sc = self.scenario
        p = self.world.native_params(seed=getattr(sc, "_seed", 0), rng_offset=self._launch_rng_offset(), scripted_ok=True)
        p.env_index_base = int(getattr(sc, "env_base", 0))
        _native.check(_native.load().fg_actor_gumbel(p, B, N, out.data_ptr(), _native.current_stream(self.world.device)))
        return out

    def _gumbel_pick(self, logits, g, explore):
        """(idx int32 [...], u [..., 2]) of logits [..., 5] and Gumbel draws g [..., 5] (None when not exploring) in the env's
        action mode (`fg_actor_gumbel_pick`: the fused kernels' pick and decode)."""
        dev = self.world.device
        logits = logits.detach().to(device=dev, dtype=torch.float32).contiguous()
        lead = tuple(logits.shape[:-1])
        idx = torch.empty(lead, dtype=torch.int32, device=dev)
        act = torch.empty(lead + (2,), dtype=torch.float32, device=dev)
        _native.check(_native.load().fg_actor_gumbel_pick(self._action_mode(), int(bool(explore)), idx.numel(), logits.data_ptr(),
                                                          _native.ptr(g), idx.data_ptr(), act.data_ptr(),
                                                          _native.current_stream(dev)))
        return idx, act

    def _categorical(self, logits, u, greedy):
        """(idx int32 [...], u [..., 2], log_prob [...]) of logits [..., 5] and draws u [...] in the env's action mode
        (`fg_actor_categorical`: the fused kernels' pick and decode)."""
        dev = self.world.device
        logits = logits.detach().to(device=dev, dtype=torch.float32).contiguous()
        lead = tuple(logits.shape[:-1])
        idx = torch.empty(lead, dtype=torch.int32, device=dev)
        act = torch.empty(lead + (2,), dtype=torch.float32, device=dev)
        logp = torch.empty(lead, dtype=torch.float32, device=dev)
        _native.check(_native.load().fg_actor_categorical(self._action_mode(), int(bool(greedy)), idx.numel(), logits.data_ptr(),
                                                          _native.ptr(u), idx.data_ptr(), act.data_ptr(), logp.data_ptr(),
                                                          _native.current_stream(dev)))
        return idx, act, logp

    def _noise_log_prob(self, eps, log_std):
        """-(eps_0^2 + eps_1^2) / 2 - sum(log_std) - log(2 pi) of eps [B, N, 2] (`fg_actor_log_prob`): [B, N]."""
        eps, log_std = eps.contiguous(), log_std.contiguous()
        out = torch.empty(eps.shape[:-1], dtype=torch.float32, device=eps.device)
        _native.check(_native.load().fg_actor_log_prob(eps.data_ptr(), log_std.data_ptr(), out.numel(), out.data_ptr(),
                                                       _native.current_stream(self.world.device)))
        return out

    def _rollout_actor_by_steps(self, K, actor, obs_every, rnn_state=None, rnn_states_every=None, noise_state=None):
        """`rollout_actor` host-paced: `actor(obs)` and `step` K times under torch.no_grad(), results stacked like the fused
        launch's (fresh tensors).  A GaussianActor: mean(obs) + exp(log_std) * eps with eps from `actor_noise`, the draws
        of the fused kernel, and the log-density from eps by the kernel's own device function (`fg_actor_log_prob`): for the
        same eps and log_std, the fused launch's bits.  A RecurrentActor (alone or as the mean): `rnn_state` [B, N, H] goes
        through the loop - a, h = actor(obs, h), then h zeroed where the step's done flag is set - is updated in place at the
        end and comes back as info['rnn_state'].  `rnn_states_every` = S: a copy of the state before the actor call of every
        step k with k % S == 0, stacked as info['rnn_states'] [ceil(K / S), B, N, state_size].  An OUNoiseActor: `noise_state`
        [B, N, 2] steps with eps from `actor_noise` by the kernels' device function (`fg_actor_ou_step`: for the same eps the
        fused launch's state bits), the action is clamp(inner(obs) + scale * x, -clip, clip), x goes back to mu where the
        step's done flag is set, is updated in place at the end and comes back as info['noise_state'].  A CategoricalActor:
        the logits from the module, the draw from `actor_uniform`, the pick and the decode by the kernels' own device functions
        (`fg_actor_categorical`), then `step` with the index (FG_ACT_INDEX) or its one-hot (FG_ACT_ONEHOT5); info['actions']
        holds the indices, info['u'] the raw actions, info['log_prob'] the log-probabilities.  A GumbelSoftmaxActor: the
        logits from the module, the draws from `actor_gumbel` while it explores, the pick and the decode by the kernels' own
        device functions (`fg_actor_gumbel_pick`), then `step` likewise; info['actions'] and info['u'], no log-probabilities."""
        ou = actor if noise_state is not None else None
        x = noise_state.clone() if ou is not None else None
        gaussian = isinstance(actor, actor_rollout.GaussianActor)
        cat = actor if isinstance(actor, actor_rollout.CategoricalActor) else None
        gumbel = actor if isinstance(actor, actor_rollout.GumbelSoftmaxActor) else None
        body = actor.mean if gaussian else actor.logits if cat is not None or gumbel is not None else actor
        picked, raw = [], []
        h = rnn_state.clone() if rnn_state is not None else None
        logp, states = [], []
        observe = getattr(self.scenario, "observe_batch", None)
        if observe is not None:                            # the observation of the current state (a multi-step launch
            observe(self.world, {"obs": self._out["obs"]})  # leaves the env's own step buffer behind)

        def mean(obs, k):                                  # a recurrent body: h goes through, a copy kept every S-th step
            nonlocal h
            if rnn_states_every is not None and k % rnn_states_every == 0:
                states.append(h.clone())
            act, h = body(obs, h)
            return act

        def sample(obs, k):                                # a GaussianActor on either body
            eps = self.actor_noise()
            ls = actor.log_std.detach().to(device=eps.device, dtype=torch.float32)
            logp.append(self._noise_log_prob(eps, ls))
            return (body(obs) if h is None else mean(obs, k)) + torch.exp(ls) * eps

        def pick(obs, k):                                  # a CategoricalActor on either body
            greedy = cat.deterministic
            idx, u_act, lp = self._categorical(body(obs) if h is None else mean(obs, k), None if greedy else self.actor_uniform(),
                                               greedy)
            picked.append(idx); raw.append(u_act); logp.append(lp)
            if self._action_mode() == _native.FG_ACT_INDEX:
                return idx
            return torch.nn.functional.one_hot(idx.long(), 5).to(torch.float32)

        def pick_gumbel(obs, k):                           # a GumbelSoftmaxActor
            exploring = gumbel.explore
            idx, u_act = self._gumbel_pick(body(obs) if h is None else mean(obs, k), self.actor_gumbel() if exploring else None, exploring)
            picked.append(idx); raw.append(u_act)
            if self._action_mode() == _native.FG_ACT_INDEX:
                return idx
            return torch.nn.functional.one_hot(idx.long(), 5).to(torch.float32)

        def explore(obs, k):                               # an OUNoiseActor
            self._ou_step(ou, self.actor_noise(), x)
            return ou.explore(ou.actor(obs), x)

        def after_step(d):                                 # an episode's end resets the states, with or without auto_reset
            nonlocal h
            if ou is not None:
                ou.reset(x, torch.as_tensor(d, device=x.device).view(torch.bool).reshape(x.shape[:-1]))
            if h is not None:
                h = h * (~torch.as_tensor(d, device=h.device).view(torch.bool).reshape(h.shape[:-1] + (1,))).to(h.dtype)

        if gaussian:
            act_fn = sample
        elif cat is not None:
            act_fn = pick
        elif gumbel is not None:
            act_fn = pick_gumbel
        elif h is not None:
            act_fn = mean
        else:
            act_fn = explore if ou is not None else lambda obs, k: actor(obs)
        with torch.no_grad():
            obs, rew, done, info = self._step_loop(K, obs_every, act_fn, after_step)
        if gaussian or cat is not None:
            info["log_prob"] = torch.stack(logp)
        if cat is not None or gumbel is not None:
            info["actions"], info["u"] = torch.stack(picked), torch.stack(raw)
        if h is not None:
            rnn_state.copy_(h)
            info["rnn_state"] = rnn_state
        if rnn_states_every is not None:
            info["rnn_states"] = torch.stack(states)
        if ou is not None:
            noise_state.copy_(x)
            info["noise_state"] = noise_state
        return obs, rew, done, info

    # ------------------------------------------------------------ buffers
    def _default_out(self, K, obs_every, policy):
        """The env's own output buffers of `rollout(out=None)` / `rollout_policy(out=None)` for this shape: placed on
        first use, kept for the next call (four shapes at most: a fifth evicts the least recently used, whose arena goes
        back to the driver with its last tensor).  The implicit probe looks at ONE arena (6 x the buffer): it never takes
        the escalation stages a caller of `alloc_rollout_buffers` may ask for (up to half of the free memory, seconds)."""
        key = (int(K), int(obs_every), bool(policy))
        out = self._auto_out.pop(key, None)
        if out is None:
            if getattr(self, "_placing", False):       # the probe's own timing launches bring their buffers
                raise RuntimeError("rollout(out=None) inside a placement probe")
            while len(self._auto_out) >= 4:
                self._auto_out.pop(next(iter(self._auto_out)))
            self._roll_launchers.clear()               # bindings keep evicted buffers alive
            out = self.alloc_rollout_buffers(K, obs_every=obs_every, policy=policy, escalate=False)
        self._auto_out[key] = out                      # most recently used last
        return out

    def _snapshot(self):
        """Everything a launch mutates (device state + host counters), for probes that must leave the env untouched."""
        w, sc = self.world, self.scenario
        dev = {k: getattr(w, k).clone() for k in ("pos_x", "pos_y", "vel_x", "vel_y", "step_count", "landmark_pos",
                                                  "obstacle_pos", "obstacle_vel")     # obstacles move; resets re-draw landmarks
               if torch.is_tensor(getattr(w, k, None))}
        scn = {k: getattr(sc, k).clone() for k in ("ideal_shape", "ideal_vel") if torch.is_tensor(getattr(sc, k, None))}
        ctr = None if w.rng_counter is None else w.rng_counter.clone()
        own = sc.snapshot_state() if hasattr(sc, "snapshot_state") else None      # a tensor scenario's per-env tensors, its generator
        return dev, scn, ctr, (self._rng_offset, self.current_step, w.world_step), own

    def _restore(self, snap):
        dev, scn, ctr, host, own = snap
        w, sc = self.world, self.scenario
        if own is not None:
            sc.restore_state(own)
        for k, v in dev.items():
            getattr(w, k).copy_(v)
        for k, v in scn.items():
            getattr(sc, k).copy_(v)
        if ctr is not None:
            w.rng_counter.copy_(ctr)
        self._rng_offset, self.current_step, w.world_step = host
        sc._cache = None

    def alloc_rollout_buffers(self, K, obs_every=1, obs_env_pitch=0, policy=False, candidates=8, mem_fraction=0.5,
                              max_arena_bytes=None, escalate=True, primed=True):
        """Output buffers for `rollout` / `rollout_policy` launches of K steps, with the observation buffer - 99 % of
        the bytes - PLACED: when it is larger than the Infinity Cache, candidate buffers are composed of the chunks of a
        small arena of device memory (6 x the buffer up to 48 GiB, at least 1.5 x the buffer, never more than
        `mem_fraction` of the free memory; `max_arena_bytes` overrides), this env's own K-step launch is timed on
        `candidates` or more of them and the fastest is kept, every other chunk released (formation_gym/placement.py: the
        rate of a launch depends on which physical memory its buffer is composed of, by 10-20 %; ~0.2 s); where the arena
        cannot be made, on up to `candidates` whole allocations.  candidates < 2 switches the probe off.  An env in a discrete
        action mode (a CategoricalActor's buffers) is timed on the same launches with the mode set aside and put back.  The env's state
        is restored afterwards, also when the probe fails.  escalate=False: one arena only (an arena whose winner gains
        nothing is otherwise followed by up to two four times larger ones).  `obs_env_pitch` (floats, 0 = contiguous) asks for padded env blocks.  The probe's report
        is left in `self.placement`.  Returns the `out` dict to pass to `rollout(..., out=out)`.  The arena lives exactly
        as long as the observation tensor (or any view of it): dropping the tensors gives the memory back.
        ZERO-PRIMED (formation_hd_env, `primed`): the observation buffer is filled with zeros once and registered
        (placement.register_primed), on every path - the arena's winner after it is mapped for good, the winner of whole
        allocations, the unprobed allocation - and each candidate of a probe before it is timed, so that the probe times the
        launch the env will really run.  Launches of silent agents into it then leave out the stores of the rows'
        communication block (whole 128-byte lines of it, `FgParams.obs_zero_primed`).  THE CONTRACT: the buffer is the env's -
        launches write it, a consumer only reads it.  Who writes into it otherwise calls `prime_rollout_buffers(out)` before
        the next launch; primed=False opts out (nothing is registered, every launch writes every byte).  A buffer, probed or
        not, keeps its registration only if the flagged launch measured at least 2 % faster on it than the unflagged one
        (self.placement["zero_primed"]: kept, flagged_ms, unflagged_ms; 12 launches)."""
        K, obs_every = int(K), int(obs_every)
        B, N = self.num_envs, self.num_agents
        D = self._out["obs"].shape[-1]
        dev = self._act.device
        f = dict(dtype=torch.float32, device=dev)
        slots = K // obs_every
        pitch = int(obs_env_pitch) if obs_env_pitch else N * D
        if pitch < N * D or pitch % 2:
            raise ValueError("obs_env_pitch must be 0 or an even number of floats >= %d" % (N * D))
        small = dict(reward=torch.empty((K, B, N), **f), indiv=torch.empty((K, B, N), **f),
                     done=torch.zeros((K, B, N), dtype=torch.uint8, device=dev))
        if policy:
            small["act"] = torch.empty((K, B, N, 2), **f)

        def shaped(flat):
            return flat.view(slots, B, pitch)[:, :, :N * D].view(slots, B, N, D)

        def alloc():
            return shaped(torch.empty(slots * B * pitch, **f))

        nbytes = slots * B * pitch * 4
        primed = bool(primed) and slots > 0 and D == 6 * N and getattr(self.scenario, "obs_zero_block", False)

        def prime(obs, keeper=None):
            # zeros once, then the registration (the pad of a padded pitch is not part of `obs`: the writers fill it)
            if primed:
                obs.zero_()
                placement.register_primed(obs if keeper is None else keeper, obs.data_ptr(), nbytes, N, B, pitch)
            return obs

        probe = not (slots == 0 or nbytes < placement.MIN_PROBE_BYTES or candidates < 2)
        if not probe and not primed:
            self.placement = {"tried": 1, "probed": False}
            return dict(small, obs=alloc())
        snap = self._snapshot()
        # a scenario without a built-in controller (the landmark scenarios: `policy` asks for the buffers of rollout_actor)
        # is timed on its open-loop rollout of zero actions - the same store stream into the candidate
        closed = policy and getattr(self.scenario, "rollout_policy_batch", None) is not None
        acts = None if closed else torch.zeros((K, B, N, 2), **f)

        per_layer = self._policy_per_layer() if closed else 0

        def time_fn(obs, keeper=None, auto=True):
            # a candidate seen for the first time (the probe's untimed first-touch launch) is primed and registered for as long
            # as the probe holds it (`keeper`: the probe's own tensor; a loser's entry goes with it)
            if auto and primed and not placement.is_primed(obs.data_ptr(), nbytes, N, B, pitch):
                prime(obs, keeper)
            out = dict(small, obs=obs)
            if closed:
                self.rollout_policy(K, per_layer, out=out, obs_every=obs_every)
            else:
                self.rollout(acts, out=out, obs_every=obs_every)
            self._roll_launchers.clear()               # one binding per candidate window: do not let them pile up

        arena = None
        self._placing = True
        # the probe's own launches take raw continuous actions (the built-in controller's, or zeros): an env in a discrete
        # action mode - whose rollout_actor buffers these are - is timed with the mode set aside, on the same store stream
        modes = (self.discrete_action_input, self.discrete_action_space, self.force_discrete_action)
        self.discrete_action_input = self.discrete_action_space = self.force_discrete_action = False
        try:
            placed = None if not probe else \
                placement.probe_arena(slots * B * pitch, lambda flat: time_fn(shaped(flat), flat), dev, trials=candidates,
                                      mem_fraction=mem_fraction, max_arena_bytes=max_arena_bytes, escalate=escalate)
            if not probe:
                obs, report = alloc(), {"tried": 1, "probed": False}
            elif placed is not None:
                flat, report, arena = placed
                obs = shaped(flat)
            else:
                obs, report = placement.probe_allocation(alloc, time_fn, nbytes, dev, candidates=candidates, mem_fraction=mem_fraction)
            # The buffer that is kept, probed or not (a probe's winner is mapped for good by now: candidates of one arena
            # mapping overlap, and their launches wrote other rows here, so zeros once more).  Then the flagged launch
            # against the unflagged one on this very buffer: the skip pays where the store stream is the bound (27 x 4096 x 20
            # placed: 10.9 against 11.9 us/step), not where the writer waves' own instruction chain is (four writer waves: a
            # buffer the Infinity Cache holds 14.1 against 11.8, an ordinary allocation 14.6 against 13.0).  The registration
            # is kept only where the flagged launch is at least 2 % faster - a tie is decided the same way every time
            # (profiles/r06_zero_skip.md).
            placement.drop_primed(obs.data_ptr(), nbytes)
            if primed:
                stream = torch.cuda.current_stream(dev)
                prime(obs)
                t_on = placement._time_launch(lambda o: time_fn(o, auto=False), obs, stream, 5)
                placement.drop_primed(obs.data_ptr(), nbytes)
                t_off = placement._time_launch(lambda o: time_fn(o, auto=False), obs, stream, 5)
                primed = t_on <= 0.98 * t_off
                report["zero_primed"] = {"kept": primed, "flagged_ms": round(t_on, 4), "unflagged_ms": round(t_off, 4)}
        finally:
            # whatever happened inside the probe (out of memory, a failed launch): the env is usable and unchanged afterwards
            self._placing = False
            self.discrete_action_input, self.discrete_action_space, self.force_discrete_action = modes
            self._roll_launchers.clear()               # bindings made on the candidates keep them alive: drop them,
            torch.cuda.empty_cache()                   # then hand the losers back to the driver
            self._restore(snap)
        if probe:
            report["buffer_MB"] = round(nbytes / 1e6, 1)
        if report.get("probed") and D == 6 * N:
            alg = _native.step_hd_bytes(N) * B * K
            report["kept_GBps"] = round(alg / (report["kept_ms"] * 1e-3) / 1e9, 1)
            report["worst_GBps"] = round(alg / (report["worst_ms"] * 1e-3) / 1e9, 1)
        self.placement = report
        return dict(small, obs=prime(obs))

    def prime_rollout_buffers(self, out):
        """Fills out["obs"] (fp32, [slots, B, N, 6N], contiguous or with a padded env pitch) with zeros and registers it as
        zero-primed again (`alloc_rollout_buffers`): for a caller that has written into the buffer, or launched a world with a
        non-silent agent into it (which drops the registration).  Returns `out`."""
        obs = out["obs"]
        B, N = self.num_envs, self.num_agents
        if not getattr(self.scenario, "obs_zero_block", False) or obs.dtype != torch.float32 or obs.dim() != 4 \
                or tuple(obs.shape[1:]) != (B, N, 6 * N):
            raise ValueError("prime_rollout_buffers: out['obs'] must be a float32 [slots, %d, %d, %d] tensor of formation_hd_env" % (B, N, 6 * N))
        pitch = self.scenario.obs_env_pitch(obs, N) or 6 * N * N
        obs.zero_()
        placement.register_primed(obs, obs.data_ptr(), ((obs.shape[0] * B - 1) * pitch + 6 * N * N) * 4, N, B, pitch)
        return out

    def _policy_per_layer(self):
        """Agents per layer of the built-in controller's hierarchy for this agent count (N = per^L): 3 where it fits (the
        reference's README.md:34-36), else the smallest of 2 ... 8 that does."""
        N = self.num_agents
        for per in (3, 2, 4, 5, 6, 7, 8):
            n = per
            while n < N:
                n *= per
            if n == N:
                return per
        raise ValueError("the built-in controller needs N = per^L agents with 2 <= per <= 8, got %d" % N)

    def place_step_buffers(self, candidates=8, mem_fraction=0.5):
        """The same placement for the per-step output buffer `step` writes into (only batches whose single-step
        observation tensor exceeds the Infinity Cache: 243 agents x >= 200 envs, 81 x >= 1700, 27 x >= 15 000)."""
        from . import placement
        B, N = self.num_envs, self.num_agents
        obs_dim = self._out["obs"].shape[-1]
        n_obs, n_bn = B * N * obs_dim, B * N
        nflat = n_obs + 2 * n_bn + (n_bn + 3) // 4
        dev = self._act.device
        if n_obs * 4 < placement.MIN_PROBE_BYTES or candidates < 2:
            self.placement = {"tried": 1, "probed": False}
            return self.placement
        extra = {k: v for k, v in self._out.items() if k not in ("obs", "reward", "indiv", "done")}

        def views(flat):
            return dict(extra, obs=flat[:n_obs].view(B, N, obs_dim), reward=flat[n_obs:n_obs + n_bn].view(B, N),
                        indiv=flat[n_obs + n_bn:n_obs + 2 * n_bn].view(B, N),
                        done=flat[n_obs + 2 * n_bn:].view(torch.uint8)[:n_bn].view(B, N))

        snap = self._snapshot()
        old_flat, self._flat, self._out = self._flat, None, None
        del old_flat
        torch.cuda.empty_cache()
        act = torch.zeros_like(self._act)

        def alloc():
            return torch.zeros(nflat, dtype=torch.float32, device=dev)

        def time_fn(flat):
            self.scenario.step_batch(self.world, act, views(flat), auto_reset=self.auto_reset, rng_offset=1)

        placed = placement.probe_arena(nflat, time_fn, dev, trials=candidates, mem_fraction=mem_fraction)
        if placed is not None:
            flat, report, arena = placed
            flat.zero_()
        else:
            flat, report = placement.probe_allocation(alloc, time_fn, nflat * 4, dev, candidates=candidates, mem_fraction=mem_fraction)
        self._flat, self._out = flat, views(flat)
        self._launchers.clear()
        self._restore(snap)
        report["buffer_MB"] = round(nflat * 4 / 1e6, 1)
        self.placement = report
        return report

    def use_device_rng_counter(self, on=True):
        """Keep the per-step offset of the device counter RNG (auto-reset draws, motor noise, and a learned actor's
        exploration draws in `rollout_actor`: a GaussianActor's and an OUNoiseActor's eps, a CategoricalActor's uniforms, a
        GumbelSoftmaxActor's Gumbel draws - the fused launches and the host-paced loop's `actor_noise()`, `actor_uniform()`,
        `actor_gumbel()` alike) in DEVICE memory (`FgParams.rng_offset_dev`) and advance it with a device-side add after
        every launch, instead of passing it by value.  Needed when the step loop - `step`, `rollout`, `rollout_policy` or a
        fused `rollout_actor` - is captured in a hipGraph (torch.cuda.CUDAGraph) with auto-reset on or an exploring actor:
        by-value launch arguments are frozen at capture, so every replay would repeat the same reset draws and the same
        exploration noise.  The draws are the same in both modes (a captured loop, replayed, equals the loop run launch by
        launch): step k of a launch draws at FgParams.rng_offset + the counter + k, a 64-bit sum, so a carry into the high
        word arrives through the counter as it does by value.  A captured `rollout_actor` reads the actor's weights
        and the states (`rnn_state`, `noise_state`) in place at every replay; what the call reads on the HOST - an
        OUNoiseActor's scalars, `deterministic`, `explore` - is frozen at capture (tests/test_gpu_actor_graph.py)."""
        if on and self.world.rng_counter is None:
            self.world.rng_counter = torch.full((1,), int(self._rng_offset), dtype=torch.int64, device=self.world.device)
        elif not on and self.world.rng_counter is not None:
            self._rng_offset = int(self.world.rng_counter.item())
            self.world.rng_counter = None
        self._launchers.clear()
        self._roll_launchers.clear()

    def _launch_rng_offset(self):
        """By-value offset of the next launch's first step: steps taken so far + 1; with the device counter that
        count lives on the device and the by-value part is the constant 1."""
        return 1 if self.world.rng_counter is not None else self._rng_offset + 1

    def _advance_rng(self, K):
        self._rng_offset += K
        if self.world.rng_counter is not None:
            self.world.rng_counter.add_(K)             # stream-ordered after the launch that read it

    def _bound_step(self, act, rng_offset):
        """Per-step host work kept to one ctypes call: the scenario resolves every pointer and the
        FgParams struct once (`bind_step`), keyed by everything the binding depends on - action
        buffer, output buffers, stream, auto-reset flag and the world's physics constants - so a
        change of any of them simply binds again.  Scenarios without `bind_step` take the generic
        path.  The world's signature covers every agent's attributes; it is cached behind a write counter
        (core._version), so the per-step key costs a few comparisons whatever the agent count."""
        bind = getattr(self.scenario, "bind_step", None)
        if bind is None:
            return False
        key = (act.data_ptr(), self.auto_reset, _native.current_stream_fast(self.world.device),
               self.world.params_signature(), getattr(self.scenario, "_seed", 0))
        launch = self._launchers.get(key)
        if launch is None:
            if len(self._launchers) >= 64:
                self._launchers.clear()
            launch = self._launchers[key] = bind(self.world, act, self._out, auto_reset=self.auto_reset)
        launch(rng_offset)
        self.scenario._cache = self._out
        return True

    def _action_mode(self):
        """Which branch of _set_action applies (environment.py:194-216); 0 = plain continuous."""
        if self.discrete_action_input:
            return _native.FG_ACT_INDEX
        if self.discrete_action_space:
            return _native.FG_ACT_ONEHOT5
        if self.force_discrete_action:
            return _native.FG_ACT_ARGMAX
        return 0

    def _decode_action_seq(self, action_seq, mode):
        """A K-step sequence in one of the discrete action modes -> raw u [K, B, N, 2] (a staging tensor of the env, re-used
        while K stays the same).  Shapes per mode as in `step`: [K,B,N,5] floats (one-hot-5 logits), [K,B,N] indices,
        [K,B,N,2] floats (force_discrete_action: the caller's array is rewritten as the one-hot, environment.py:213-215)."""
        B, N = self.num_envs, self.num_agents
        dev = self.world.device
        tail, dtype = {_native.FG_ACT_ONEHOT5: ((B, N, 5), torch.float32),
                       _native.FG_ACT_INDEX: ((B, N), torch.int32),
                       _native.FG_ACT_ARGMAX: ((B, N, 2), torch.float32)}[mode]
        if not torch.is_tensor(action_seq) or tuple(action_seq.shape[1:]) != tail or action_seq.dim() != len(tail) + 1:
            raise ValueError("action_seq must be a tensor of shape [K%s] in this action mode" % "".join(", %d" % d for d in tail))
        K = int(action_seq.shape[0])
        src = action_seq
        if src.dtype != dtype or src.device != dev or not src.is_contiguous():
            src = src.to(device=dev, dtype=dtype).contiguous()
        stage = getattr(self, "_act_seq_stage", None)
        if stage is None or stage.shape[0] != K:
            stage = self._act_seq_stage = torch.empty((K, B, N, 2), dtype=torch.float32, device=dev)
        if K:
            _native.check(_native.load().fg_decode_actions(mode, K * B * N, src.data_ptr(), stage.data_ptr(),
                                                           _native.current_stream(dev)))
        if mode == _native.FG_ACT_ARGMAX and src is not action_seq:
            action_seq.copy_(src)                      # the reference overwrites the caller's array (:213-215)
        return stage

    def _decode_actions(self, action_n, mode, batched):
        """Non-default action modes: stage the caller's actions on the device ([B,N,5] floats,
        [B,N] indices or [B,N,2] floats) and decode them to raw u with `fg_decode_actions`."""
        B, N = self.num_envs, self.num_agents
        dev = self.world.device
        shape, dtype = {_native.FG_ACT_ONEHOT5: ((B, N, 5), torch.float32),
                        _native.FG_ACT_INDEX: ((B, N), torch.int32),
                        _native.FG_ACT_ARGMAX: ((B, N, 2), torch.float32)}[mode]
        if batched:
            if tuple(action_n.shape) != shape:
                raise ValueError("batched action must have shape %s in this action mode, got %s"
                                 % (shape, tuple(action_n.shape)))
            src = action_n
            if src.dtype != dtype or src.device != dev or not src.is_contiguous():
                src = src.to(device=dev, dtype=dtype).contiguous()
        else:
            if B != 1:
                raise ValueError("a list of per-agent actions needs num_envs == 1; pass a batched tensor")
            if len(action_n) != N:
                raise ValueError("expected %d agent actions, got %d" % (N, len(action_n)))
            host = np.asarray([np.asarray(a) for a in action_n]).reshape((1,) + shape[1:])
            src = torch.as_tensor(host).to(device=dev, dtype=dtype).contiguous()
        _native.check(_native.load().fg_decode_actions(mode, B * N, src.data_ptr(), self._act.data_ptr(),
                                                       _native.current_stream(self.world.device)))
        if mode == _native.FG_ACT_ARGMAX:
            if batched:
                if src is not action_n:
                    action_n.copy_(src)           # the reference overwrites the caller's array (:213-215)
            else:
                sens = [a.accel if a.accel is not None else 5.0 for a in self.agents]
                onehot = src[0].cpu().numpy()
                for i, a in enumerate(action_n):  # ... and scales it through the `u` view (:216,:221)
                    if isinstance(a, np.ndarray):
                        a[:] = 0.0
                        a[0:2] = onehot[i] * sens[i]
        return self._act

    def _stage_reference_actions(self, action_n):
        """environment.py:121-122,187-236 for the continuous path, B == 1."""
        if self.num_envs != 1:
            raise ValueError("a list of per-agent actions needs num_envs == 1; pass a [B,N,2] tensor")
        if len(action_n) != self.num_agents:
            raise ValueError("expected %d agent actions, got %d" % (self.num_agents, len(action_n)))
        pinned = self._act_host is not None
        host = self._act_host.numpy() if pinned else np.empty((1, self.num_agents, 2), dtype=np.float32)
        for i, (a, agent) in enumerate(zip(action_n, self.agents)):
            if isinstance(a, (list, tuple)):
                # the reference fails at `agent.action.u *= sensitivity` (:221)
                raise TypeError("can't multiply sequence by non-int of type 'float'")
            a = a if isinstance(a, np.ndarray) else np.asarray(a)
            host[0, i] = a[0:2]
            sens = agent.accel if agent.accel is not None else 5.0
            a[0:2] *= sens            # the reference scales the caller's array in place (:216,:221)
        if pinned:         # the previous step's copy has completed: every reference-style step ends with a stream sync
            self._act.copy_(self._act_host, non_blocking=True)
        else:
            self._act.copy_(torch.from_numpy(host))
        return self._act

    def _batched_result(self):
        o = self._out
        rew = o["reward"].unsqueeze(-1)
        if not self.shared_reward:
            first = getattr(self.scenario, "first_reward", None)      # a reference-style Scenario file: environment.py:128 vs :130
            rew = (o["indiv"] if first is None else first).unsqueeze(-1)
        return o["obs"], rew, o["done"].view(torch.bool), {"individual_reward": o["indiv"]}   # 0/1 bytes: a view, no kernel

    def _reference_result(self):
        o = self._out
        N = self.num_agents
        if self._host is not None:        # one pinned device-to-host copy + one stream sync for the whole step
            self._host.copy_(self._flat, non_blocking=True)
            torch.cuda.current_stream(self._flat.device).synchronize()
            h = self._host.numpy()
            n_obs = o["obs"].numel()
            obs = h[:n_obs].reshape(N, -1).astype(np.float64)
            shared = float(h[n_obs])
            indiv = h[n_obs + N:n_obs + 2 * N].astype(np.float64)
            done = bool(h[n_obs + 2 * N:].view(np.uint8)[0])
        else:
            obs = o["obs"][0].double().cpu().numpy()
            indiv = o["indiv"][0].double().cpu().numpy()
            shared = float(o["reward"][0, 0].double().cpu())
            done = bool(o["done"][0, 0].cpu())
        obs_n = [obs[i] for i in range(N)]
        if self.shared_reward:
            reward_n = [[shared]] * N                     # :136-138
        else:
            first = getattr(self.scenario, "first_reward", None)      # see _batched_result
            per_agent = indiv if first is None else first[0].double().cpu().numpy()
            reward_n = [[float(per_agent[i])] for i in range(N)]
        done_n = [done] * N
        info_n = [{'individual_reward': float(indiv[i])} for i in range(N)]
        return obs_n, reward_n, done_n, info_n

    # ----------------------------------------------------------------- reset
    def reset(self, batched=None):
        """environment.py:144-156.  Returns a list of N float64 arrays when
        num_envs == 1 (reference style) unless batched=True; else obs [B,N,D]."""
        self.current_step = 0
        self.reset_callback(self.world)
        self.agents = self.world.policy_agents
        self.scenario.observe_batch(self.world, self._out)
        if batched is None:
            batched = self.num_envs != 1
        if batched:
            return self._out["obs"]
        obs = self._out["obs"][0].double().cpu().numpy()
        return [obs[i] for i in range(self.num_agents)]

    # ---------------------------------------------------- per-agent callbacks
    def _get_info(self, agent):
        if self.info_callback is None:
            return {}
        return self.info_callback(agent, self.world)

    def _get_obs(self, agent):
        if self.observation_callback is None:
            return np.zeros(0)
        return self.observation_callback(agent, self.world)

    def _get_done(self, agent):
        if self.done_callback is None:
            return self.current_step >= self.world_length
        return self.done_callback(agent, self.world)

    def _get_reward(self, agent):
        if self.reward_callback is None:
            return 0.0
        return self.reward_callback(agent, self.world)

    def render(self, mode='human', close=False):
        raise NotImplementedError("the pyglet renderer of the reference (environment.py:243-393) "
                                  "is out of scope for the MI355X hot path")

    def close(self):
        """Drop the env's own placed buffers and bound launches: their arenas go back to the driver with the last tensor."""
        self._auto_out.clear()
        self._roll_launchers.clear()
        self._launchers.clear()
        self.scenario._cache = None
