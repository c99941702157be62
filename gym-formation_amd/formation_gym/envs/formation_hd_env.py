"""formation_hd_env: Hausdorff-distance formation task (reference
formation_gym/envs/formation_hd_env.py), MI355X-native.

Same plugin surface (`class Scenario(BaseScenario)` with make_world /
reset_world / observation / reward / benchmark_data / is_collision /
generate_shape).  The arithmetic of observation (:38-59), reward (:61-75) and
the env shell's done (environment.py:172-178) runs inside the fused HIP kernel
`fg_step_hd`; the per-agent callbacks return that agent's slice.
"""
import ctypes

import numpy as np
import torch

from formation_gym import _native, placement
from formation_gym.core import World, Agent, Landmark
from formation_gym.scenario import BaseScenario


class _Plan(object):
    """Owner of a library-side launch plan (fg_step_hd_plan): keeps the tensors whose addresses the plan holds alive and
    frees the plan with the last reference to the bound launcher."""

    def __init__(self, lib, handle, keep):
        self.lib, self.handle, self.keep = lib, handle, keep

    def __del__(self):
        try:
            if self.handle:
                self.lib.fg_plan_destroy(self.handle)
                self.handle = None
        except Exception:                 # noqa: BLE001 - interpreter shutdown
            pass


class Scenario(BaseScenario):
    # observation rows carry a communication block that is zero for silent agents: the env's rollout buffers are filled
    # with zeros once and registered (placement.register_primed), see `params`
    obs_zero_block = True

    def make_world(self, num_agents=3, episode_length=100, num_envs=1, device=None):
        world = World(num_envs=num_envs, device=device)
        world.world_length = episode_length
        world.dim_c = 2
        world.collaborative = True
        self.num_agents = num_agents
        world.agents = [Agent() for _ in range(num_agents)]
        for i, agent in enumerate(world.agents):
            agent.name = 'agent %d' % i
            agent.collide = True
            agent.silent = True
            agent.size = 0.03
        world.landmarks = [Landmark() for _ in range(num_agents)]
        for i, landmark in enumerate(world.landmarks):
            landmark.name = 'landmarks %d' % i
            landmark.collide = False
            landmark.movable = False
            landmark.size = 0.01
        world.allocate()
        world.scenario = self
        B, N = world.num_envs, num_agents
        f = dict(dtype=torch.float32, device=world.device)
        self.ideal_shape = torch.zeros((B, N, 2), **f)     # Scenario attribute, as in :86-93
        self.ideal_vel = torch.zeros((B, 2), **f)          # :95
        self._rngs = None
        self._seed = 1
        self._cache = None
        self.reset_world(world)
        return world

    # ---- RNG: the reference draws from the global legacy MT19937 ----------
    def seed(self, seed=None):
        """env.seed(s) (environment.py:106-110).  Env b gets RandomState(s + 1000 (env_base + b)),
        the per-worker convention of train/maddpg-v2/main.py:19-30; b = 0 is the
        reference's single env.  `env_base` = global index of this batch's env 0 (sharding.make_env_shard)."""
        self._seed = 1 if seed is None else int(seed)
        self._rngs = None
        self._mt_state = None

    def _streams(self, B):
        if self._rngs is None or len(self._rngs) != B:
            self._rngs = [np.random.RandomState(self._seed + 1000 * (getattr(self, "env_base", 0) + b)) for b in range(B)]
        return self._rngs

    def reset_world(self, world, env_mask=None):
        """:77-95 - N agent positions, N landmark positions, one ideal velocity,
        each U(-1,1)^2, drawn in that order from each env's own stream; the
        ideal shape is the centred landmark set."""
        B, N = world.num_envs, len(world.agents)
        rngs = self._streams(B)
        idx = range(B) if env_mask is None else [b for b in range(B) if env_mask[b]]
        pos, vel = world.get_state()
        pos = pos.cpu().numpy().astype(np.float64); vel = vel.cpu().numpy().astype(np.float64)
        shape = self.ideal_shape.cpu().numpy().astype(np.float64)
        ivel = self.ideal_vel.cpu().numpy().astype(np.float64)
        lm = world.landmark_pos.cpu().numpy().astype(np.float64)
        for b in idx:
            rs = rngs[b]
            pos[b] = rs.uniform(-1, +1, (N, 2))
            vel[b] = 0.0
            raw = rs.uniform(-1, +1, (N, 2))
            shape[b] = raw - raw.mean(0)
            lm[b] = raw
            ivel[b] = rs.uniform(-1, +1, 2)
        world.set_state(pos, vel)
        self.ideal_shape.copy_(torch.as_tensor(shape, dtype=torch.float32))
        self.ideal_vel.copy_(torch.as_tensor(ivel, dtype=torch.float32))
        world.landmark_pos.copy_(torch.as_tensor(lm, dtype=torch.float32))
        if env_mask is None:
            world.step_count.zero_()
        else:
            m = torch.as_tensor(np.asarray(env_mask, dtype=bool), device=world.device)
            world.step_count.masked_fill_(m, 0)
        self._cache = None

    def set_formation(self, world, ideal_shape=None, ideal_vel=None):
        """Upload explicit ideal shapes [B,N,2] / velocities [B,2] (parity tests, curricula)."""
        if ideal_shape is not None:
            self.ideal_shape.copy_(torch.as_tensor(np.array(ideal_shape), dtype=torch.float32))
        if ideal_vel is not None:
            self.ideal_vel.copy_(torch.as_tensor(np.array(ideal_vel), dtype=torch.float32))
        self._cache = None

    # ---- batched protocol ----------------------------------------------------
    def obs_dim(self, world):
        return 6 * len(world.agents)

    def params(self, world, auto_reset=False, rng_offset=0, obs=None, scripted_ok=False):
        """The FgParams of a launch of this world into `obs`.  NOT free of side effects where `obs` touches a zero-primed
        buffer (placement.register_primed): params are built for a launch that is about to write `obs`, so a non-silent world,
        a 16-bit `obs` or a view that does not start on a step slot of the registered buffer DROPS that buffer's registration -
        also when the caller only describes the launch (`fg_describe_launch`) or never runs it.  That errs on the safe side:
        `env.prime_rollout_buffers(out)` registers the buffer again."""
        a0 = world.agents[0]
        p = world.native_params(collide_thresh=(a0.size + a0.size) / 2,   # :121
                                auto_reset=auto_reset, seed=self._seed, rng_offset=rng_offset, scripted_ok=scripted_ok)
        p.obs_env_pitch = self.obs_env_pitch(obs, len(world.agents))
        p.env_index_base = int(getattr(self, "env_base", 0))
        if world.any_non_silent():                        # :48-51 the communication block carries the others' state.c
            if world.dim_c != 2:
                raise NotImplementedError("formation_hd_env's observation has a communication block of dim_c = 2 (:40, :48-51); "
                                          "World.step / update_agent_state take any dim_c")
            comm = world.ensure_comm()[0]
            p.comm_state = comm.data_ptr()
            p._pinned += (comm,)                          # as native_params pins its own: whoever keeps p keeps the tensor
        if obs is not None and obs.numel() and placement.is_placed(obs.data_ptr()):
            p.obs_placed = 1                              # a buffer of chunks spread over the device memory: more writer waves pay
        # (host cost: params are built per launch on the unbound paths - nothing below runs unless a registered buffer is near)
        if obs is None or not placement.near_primed(obs):
            pass
        elif p.comm_state or obs.dtype != torch.float32:
            # this launch writes the communication block, or 16-bit rows (another layout): no longer zeros where they were
            placement.drop_primed(obs.data_ptr(), obs.numel() * obs.element_size())
        else:
            # a buffer alloc_rollout_buffers made, filled with zeros once and registered: the communication blocks of
            # silent agents still hold those zeros, and the tile writers leave their whole 128-byte lines out
            N = len(world.agents)
            pitch = p.obs_env_pitch or 6 * N * N
            if placement.is_primed(obs.data_ptr(), self._obs_extent(obs, p.obs_env_pitch, N), N, world.num_envs, pitch, launch=True):
                p.obs_zero_primed = 1
        return p

    @staticmethod
    def _obs_extent(obs, env_pitch, N):
        """Bytes from the first to behind the last env block of an observation tensor [.., B, N, 6N] (env_pitch floats
        apart, 0 = contiguous)."""
        blocks = obs.numel() // (6 * N * N)
        return ((blocks - 1) * (env_pitch or 6 * N * N) + 6 * N * N) * obs.element_size()

    @staticmethod
    def obs_env_pitch(obs, N):
        """Floats between the [N, 6N] blocks of consecutive envs of an observation tensor [B, N, 6N] or
        [K, B, N, 6N]: 0 for a contiguous tensor, else its (padded) env stride.  Rows must be dense and, with a step
        axis, the step slots B env pitches apart - anything else cannot be described to the kernels."""
        if obs is None or obs.numel() == 0 or obs.is_contiguous():
            return 0
        D = 6 * N
        ok = obs.dim() in (3, 4) and obs.stride(-1) == 1 and obs.stride(-2) == D and obs.shape[-2:] == (N, D)
        B = obs.shape[-3] if ok else 0
        slots = obs.shape[0] if ok and obs.dim() == 4 else 1
        # a dimension of size 1 has no meaningful stride: the pitch is read from whichever of (env, step slot) moves
        if ok and B > 1:
            pitch = obs.stride(-3)
            if slots > 1:
                ok = obs.stride(0) == B * pitch
        elif ok and slots > 1:
            pitch = obs.stride(0)                    # one env per slot: slots are one pitch apart
        else:
            pitch = N * D
        if not ok or pitch < N * D or pitch % 2:
            raise ValueError("observation tensor must be [.., B, N, 6N] with dense rows and a uniform even env pitch "
                             ">= 6 N^2 floats; got shape %s strides %s" % (tuple(obs.shape), tuple(obs.stride())))
        if pitch == N * D:
            return 0
        return int(pitch)

    def _state_ptrs(self, world, act):
        """The world state as every step / rollout entry takes it, the action (sequence) tensor `act` in its place."""
        return (world.pos_x.data_ptr(), world.pos_y.data_ptr(), world.vel_x.data_ptr(), world.vel_y.data_ptr(),
                act.data_ptr(), self.ideal_shape.data_ptr(), self.ideal_vel.data_ptr(), world.step_count.data_ptr())

    @staticmethod
    def _out_ptrs(out):
        """The outputs every step / rollout entry writes, in the entries' order (the reward alone is required)."""
        return (_native.ptr(out.get("obs")), out["reward"].data_ptr(), _native.ptr(out.get("indiv")),
                _native.ptr(out.get("done")))

    def _step_args(self, world, act, out):
        """The arguments of `fg_step_hd` / `fg_step_hd_plan` after the FgParams struct."""
        return (world.num_envs, len(world.agents)) + self._state_ptrs(world, act) + self._out_ptrs(out) + (
            _native.ptr(out.get("near_lm")), _native.ptr(out.get("near_ag")), _native.ptr(out.get("hd_idx")),
            _native.current_stream(world.device))

    def step_batch(self, world, act, out, auto_reset=False, rng_offset=0):
        _native.check(_native.load().fg_step_hd(self.params(world, auto_reset, rng_offset, out.get("obs")),
                                                *self._step_args(world, act, out)))
        self._cache = out

    def bind_step(self, world, act, out, auto_reset=False):
        """Resolve every pointer once and return `launch(rng_offset)`: the per-call
        host work is one ctypes call (rollout loops, bench.py)."""
        lib = _native.load()
        p = self.params(world, auto_reset, 0, out.get("obs"))
        args = self._step_args(world, act, out)
        # the checked launch description is kept by the library (fg_step_hd_plan): a step is a two-argument call
        handle = ctypes.c_void_p()
        _native.check(lib.fg_step_hd_plan(p, *args, ctypes.byref(handle)))
        plan = _Plan(lib, handle, (act, out, p, world.pos_x, world.pos_y, world.vel_x, world.vel_y, self.ideal_shape,
                                   self.ideal_vel, world.step_count))
        fn = lib.fg_plan_launch
        raw = plan.handle

        def launch(rng_offset=0):
            rc = fn(raw, rng_offset)
            if rc:
                _native.check(rc)
            return plan
        self._cache = None
        return launch

    def observe_batch(self, world, out):
        lib = _native.load()
        _native.check(lib.fg_observe_hd(                      # (no action involved: a World with scripted agents may be observed)
            self.params(world, obs=out.get("obs"), scripted_ok=True), world.num_envs, len(world.agents),
            world.pos_x.data_ptr(), world.pos_y.data_ptr(), world.vel_x.data_ptr(), world.vel_y.data_ptr(),
            self.ideal_shape.data_ptr(), self.ideal_vel.data_ptr(), world.step_count.data_ptr(),
            _native.ptr(out.get("obs")), _native.ptr(out.get("reward")), _native.ptr(out.get("indiv")),
            _native.ptr(out.get("done")), _native.ptr(out.get("near_lm")), _native.ptr(out.get("near_ag")),
            _native.ptr(out.get("hd_idx")), _native.current_stream(world.device)))
        self._cache = out

    def obs16_supported(self, world, K, per_layer=0):
        """Whether a K-step launch (per_layer 0: `rollout_batch`, else `rollout_policy_batch`) of this world can store its
        observations in fp16 / bf16 itself (`obs_format`): the library's own answer (`fg_describe_obs16_launch`, which touches
        no device).  False: the caller runs the fp32 launch and casts."""
        try:
            p = self.params(world)
        except NotImplementedError:                        # scripted agents: only the World API drives them
            return False
        buf = ctypes.create_string_buffer(256)
        return _native.load().fg_describe_obs16_launch(p, _native.FG_OBS_F16, world.num_envs, len(world.agents), int(K),
                                                       int(per_layer), 1, buf, len(buf)) == _native.FG_OK

    @staticmethod
    def _rollout_entry(lib, name, obs_format):
        """(C entry, its arguments between params and B) of a K-step launch: `name`, or its 16-bit twin with the format."""
        return (getattr(lib, name + "_obs16"), (int(obs_format),)) if obs_format else (getattr(lib, name), ())

    def rollout_batch(self, world, act_seq, out, obs_every=1, auto_reset=False, rng_offset=0, obs_format=0):
        """K steps in one launch; act_seq [K,B,N,2], out tensors carry a leading K.  obs_format (_native.FG_OBS_F16 / _BF16):
        out["obs"] is a contiguous tensor of that 16-bit dtype, written by the launch itself (`fg_rollout_hd_obs16`)."""
        self.bind_rollout(world, act_seq, out, obs_every, auto_reset, obs_format)(rng_offset)
        self._cache = None

    def rollout_policy_batch(self, world, K, per_layer, out, obs_every=1, auto_reset=False, rng_offset=0, obs_format=0):
        """K closed-loop steps with the built-in controller (`fg_rollout_hd_policy`): out["act"] [K,B,N,2]
        receives the actions taken, the other tensors (and obs_format) are those of `rollout_batch`."""
        self.bind_rollout_policy(world, K, per_layer, out, obs_every, auto_reset, obs_format)(rng_offset)
        self._cache = None

    def bind_rollout_policy(self, world, K, per_layer, out, obs_every=1, auto_reset=False, obs_format=0):
        """`rollout_policy_batch` with every pointer and the FgParams struct resolved once: returns
        `launch(rng_offset)`, one ctypes call per closed-loop launch."""
        lib = _native.load()
        p = self.params(world, auto_reset, 0, out.get("obs"))
        fn, fmt = self._rollout_entry(lib, "fg_rollout_hd_policy", obs_format)
        args = fmt + (world.num_envs, len(world.agents), int(K), int(per_layer)) + self._state_ptrs(world, out["act"]) \
            + self._out_ptrs(out) + (int(obs_every), _native.current_stream(world.device))
        return _native.bind_launch(fn, p, *args, keep=out)

    def actor_obs16_supported(self, world, K, actor, act_mode=0):
        """Whether a K-step `bind_rollout_actor` launch of this world with `actor` (a FusedActor record) can store its
        observations in fp16 / bf16 itself (`obs_format`): the Gaussian and the categorical member of the plain, the LayerNorm
        and the recurrent family, by the library's own answer (`fg_describe_actor_obs16_launch` /
        `fg_describe_actor_cat_obs16_launch`, which touch no device).  False: the caller runs the fp32 launch and casts."""
        if actor.ou is not None or actor.per_agent or (actor.cat is None and actor.log_std is None):
            return False
        try:
            p = self.params(world)
        except NotImplementedError:                        # scripted agents: only the World API drives them
            return False
        fas, norm, gru, bns = _native.actor_structs(actor)
        if bns is not None:
            return False
        lib, buf = _native.load(), ctypes.create_string_buffer(256)
        shape = (world.num_envs, len(world.agents), int(K), 1, buf, len(buf))
        if actor.cat is not None:
            rc = lib.fg_describe_actor_cat_obs16_launch(p, _native.FG_OBS_F16, fas, norm, gru, int(act_mode), 0, *shape)
        else:
            rc = lib.fg_describe_actor_obs16_launch(p, _native.FG_OBS_F16, fas, norm, gru, _native.ptr(actor.log_std), *shape)
        return rc == _native.FG_OK

    def bind_rollout_actor(self, world, K, actor, out, obs_every=1, auto_reset=False, rnn_state=None, rnn_states_every=None,
                           noise_state=None, act_mode=0, obs_format=0):
        """K closed-loop steps with the caller's MLP actor, every pointer and the FgParams struct resolved once: returns
        `launch(rng_offset)`.  `actor`: the FusedActor record of `actor_rollout.resolve_actor`; the kernel reads its tensors
        in place at every launch, and the launcher keeps them alive.  out["act"] [K,B,N,2] receives the actions taken, the
        other tensors are those of `rollout_batch`.  The entry points (the `families` list below, last row first):
          one shared actor                      `fg_rollout_hd_actor`
          ... with a GaussianActor's log_std    `fg_rollout_hd_actor_sample`, the log-densities in out["log_prob"] [K,B,N]
          one actor per agent                   `fg_rollout_hd_actor_per_agent` (log_std or NULL), agent i's rows through
                                                member i's weights
          one shared actor with LayerNorms      `fg_rollout_hd_actor_norm` (log_std or NULL), `actor.norms` as FgActorNorm
          ... with a recurrent layer            `fg_rollout_hd_actor_gru` (log_std or NULL), `actor.gru` as FgActorGru and
                                                `rnn_state` [B,N,H], read and updated in place by every launch and kept alive
                                                by the launcher like the GRU's tensors
          ... that keeps its states             `fg_rollout_hd_actor_gru_states` with `rnn_states_every` = S: the state every
                                                S-th step acted with into out["rnn_states"] [ceil(K / S),B,N,H]
          an eval-mode input BatchNorm          `fg_rollout_hd_actor_bn` (shared) / `fg_rollout_hd_actor_bn_per_agent` (log_std or
                                                NULL), `actor.in_bn` as one FgActorInBn or a host array of N; the running
                                                statistics are read in place and kept alive like the weights
          an OUNoiseActor (`actor.ou`)          `fg_rollout_hd_actor_ou` / `fg_rollout_hd_actor_ou_per_agent` on the plain or the
                                                BatchNorm actor (in_bn or NULL), `noise_state` [B,N,2] read and updated in place
                                                like `rnn_state`; the FgActorOu struct is filled from the module's scalars
                                                before every launch, so a scale annealed between calls needs no new binding
          a CategoricalActor (`actor.cat`)      `fg_rollout_hd_actor_cat` on the plain, the LayerNorm or the recurrent body
                                                (norm / gru or NULL) in the env's action mode `act_mode`: the indices in
                                                out["idx"] [K,B,N] int32, the log-probs in out["log_prob"], the decoded actions
                                                in out["act"]; `rnn_state` and out["rnn_states"] as above; the module's
                                                `deterministic` flag is read before every launch
          a GumbelSoftmaxActor (`actor.gumbel`) `fg_rollout_hd_actor_gumbel` / `fg_rollout_hd_actor_gumbel_per_agent` on the plain or
                                                the BatchNorm body (in_bn or NULL) in the env's action mode `act_mode`: the
                                                indices in out["idx"] [K,B,N] int32, the decoded actions in out["act"]; the
                                                module's `explore` flag is read before every launch
          16-bit observations (`obs_format`)    `fg_rollout_hd_actor_obs16` (a GaussianActor on the plain, the LayerNorm or the
                                                recurrent body: norm / gru or NULL, log_std required, rnn_states or NULL) and
                                                `fg_rollout_hd_actor_cat_obs16` (a CategoricalActor likewise): out["obs"] is a
                                                contiguous tensor of that 16-bit dtype, written by the launch itself; where
                                                `actor_obs16_supported` says no, the library refuses and the caller casts"""
        lib = _native.load()
        log_std = actor.log_std
        fas, norm, gru, bns = _native.actor_structs(actor)
        if gru is not None and rnn_state is None:
            raise ValueError("a recurrent actor's launch needs its rnn_state")
        if rnn_states_every is not None and gru is None:
            raise ValueError("rnn_states_every needs a recurrent actor")
        if bns is not None and (norm is not None or gru is not None):
            raise NotImplementedError("an input BatchNorm fuses in front of the plain body only")
        ou = actor.ou
        if ou is not None and (norm is not None or gru is not None or log_std is not None):
            raise NotImplementedError("OU noise fuses on a deterministic actor without LayerNorms only")
        if ou is not None and noise_state is None:
            raise ValueError("an OUNoiseActor's launch needs its noise_state")
        fou = None if ou is None else _native.actor_ou(ou)
        p = self.params(world, auto_reset, 0, out.get("obs"))
        state = (world.num_envs, len(world.agents), int(K)) + self._state_ptrs(world, out["act"]) + self._out_ptrs(out)
        tail = (int(obs_every), _native.current_stream(world.device))
        cat, gumbel = actor.cat, actor.gumbel
        if gumbel is not None:
            if cat is not None or ou is not None or norm is not None or gru is not None or log_std is not None or obs_format:
                raise NotImplementedError("a GumbelSoftmaxActor fuses on the plain and the BatchNorm body, shared or per agent, with "
                                          "fp32 observations only")
        elif cat is not None:
            if ou is not None or bns is not None or actor.per_agent or log_std is not None:
                raise NotImplementedError("a CategoricalActor fuses on the plain, the LayerNorm and the recurrent body only")
        elif (gru is not None and norm is None) or (norm is not None and actor.per_agent):
            raise NotImplementedError("PerAgentActor members with LayerNorms or a recurrent layer have no fused launch")
        elif obs_format and (ou is not None or bns is not None or actor.per_agent or log_std is None):
            raise NotImplementedError("16-bit observations fuse with a Gaussian or categorical actor on the plain, the LayerNorm "
                                      "and the recurrent body only")
        # What may follow the state block: the indices, the log-probs, the hidden state, the kept states with their stride
        # (NULL and 1 where none are kept)
        keep_states = rnn_states_every is not None
        idx = (out["idx"].data_ptr(),) if cat is not None or gumbel is not None else ()
        logp = (None if cat is None and log_std is None else out["log_prob"].data_ptr(),)
        rnn = (_native.ptr(rnn_state) if gru is not None else None,)
        states = (out["rnn_states"].data_ptr() if keep_states else None, int(rnn_states_every) if keep_states else 1)
        # The families, the first that applies giving the launch: (applies, C entry, its arguments before the state, what follows
        # the state).  A categorical entry takes `greedy` as its last leading argument and a Gumbel entry `explore`, one bound
        # launch per value.
        ls, nst = _native.ptr(log_std), _native.ptr(noise_state)
        fmt, x16 = ((int(obs_format),), "_obs16") if obs_format else ((), "")
        families = (
            (gumbel is not None and actor.per_agent, "fg_rollout_hd_actor_gumbel_per_agent", (fas, bns, int(act_mode)), idx),
            (gumbel is not None, "fg_rollout_hd_actor_gumbel", (fas, bns, int(act_mode)), idx),
            (cat is not None, "fg_rollout_hd_actor_cat" + x16, fmt + (fas, norm, gru, int(act_mode)), idx + logp + rnn + states),
            (bool(obs_format), "fg_rollout_hd_actor_obs16", fmt + (fas, norm, gru, ls), logp + rnn + states),
            (ou is not None and actor.per_agent, "fg_rollout_hd_actor_ou_per_agent", (fas, bns, fou, nst), ()),
            (ou is not None, "fg_rollout_hd_actor_ou", (fas, bns, fou, nst), ()),
            (bns is not None and actor.per_agent, "fg_rollout_hd_actor_bn_per_agent", (fas, bns, ls), logp),
            (bns is not None, "fg_rollout_hd_actor_bn", (fas, bns, ls), logp),
            (keep_states, "fg_rollout_hd_actor_gru_states", (fas, norm, gru, ls), logp + rnn + states),
            (gru is not None, "fg_rollout_hd_actor_gru", (fas, norm, gru, ls), logp + rnn),
            (norm is not None, "fg_rollout_hd_actor_norm", (fas, norm, ls), logp),
            (actor.per_agent, "fg_rollout_hd_actor_per_agent", (fas, ls), logp),
            (log_std is not None, "fg_rollout_hd_actor_sample", (fas, ls), logp),
            (True, "fg_rollout_hd_actor", (fas,), ()))
        entry, lead, after = next(row[1:] for row in families if row[0])
        args = state + after + tail
        keep = (out, actor.tensors(), fas, norm, gru, bns, fou, rnn_state, noise_state)
        if cat is not None:
            by_flag = [_native.bind_launch(getattr(lib, entry), p, *lead, greedy, *args, keep=keep) for greedy in (0, 1)]

            def launch_cat(rng_offset=0):              # the module's flag as it is now: sampled or the distribution's mode
                return by_flag[1 if cat.deterministic else 0](rng_offset)
            return launch_cat
        if gumbel is not None:
            by_flag = [_native.bind_launch(getattr(lib, entry), p, *lead, explore, *args, keep=keep) for explore in (0, 1)]

            def launch_gumbel(rng_offset=0):           # the module's flag as it is now: exploring or the largest logit
                return by_flag[1 if gumbel.explore else 0](rng_offset)
            return launch_gumbel
        launch = _native.bind_launch(getattr(lib, entry), p, *lead, *args, keep=keep)
        if ou is None:
            return launch

        def launch_ou(rng_offset=0):                   # the module's scalars as they are now, into the struct the launch reads
            _native.actor_ou(ou, fou)
            return launch(rng_offset)
        return launch_ou

    def policy_actions(self, world, per_layer, out=None):
        """get_action_BFS(ezpolicy, obs, per_layer) for the CURRENT state of every env, straight from the
        simulator state (`fg_policy_bfs_state`): raw actions [B, N, 2]."""
        B, N = world.num_envs, len(world.agents)
        if out is None:
            out = torch.empty((B, N, 2), dtype=torch.float32, device=world.device)
        _native.check(_native.load().fg_policy_bfs_state(
            B, N, int(per_layer), world.pos_x.data_ptr(), world.pos_y.data_ptr(),
            self.ideal_shape.data_ptr(), self.ideal_vel.data_ptr(), out.data_ptr(),
            _native.current_stream(world.device)))
        return out

    def bind_rollout(self, world, act_seq, out, obs_every=1, auto_reset=False, obs_format=0):
        """`rollout_batch` with every pointer and the FgParams struct resolved once: returns
        `launch(rng_offset)`, one ctypes call per K-step launch (a 9 x 4096 launch lasts ~35 us on the GPU,
        less than the generic path spends in Python)."""
        lib = _native.load()
        p = self.params(world, auto_reset, 0, out.get("obs"))
        fn, fmt = self._rollout_entry(lib, "fg_rollout_hd", obs_format)
        args = fmt + (world.num_envs, len(world.agents), int(act_seq.shape[0])) + self._state_ptrs(world, act_seq) \
            + self._out_ptrs(out) + (int(obs_every), _native.current_stream(world.device))
        return _native.bind_launch(fn, p, *args, keep=(act_seq, out))

    def bind_rollout_returns(self, world, act_seqs, out, gamma=1.0):
        """The discounted returns of C candidate action sequences from the current state (`fg_rollout_hd_returns`), every
        pointer and the FgParams struct resolved once: returns `launch(rng_offset)` (the offset is ignored: the launch draws
        nothing).  act_seqs [C,K,B,N,2] raw actions; out["ret"] / out["indiv"] [C,B,N] fp32 and out["steps"] [B] int32 receive
        the shared and the individual return and the counted steps.  The launch reads the world's state and writes only `out`."""
        lib = _native.load()
        p = self.params(world)                            # no observation buffer: nothing of the zero-primed registry is touched
        args = (world.num_envs, len(world.agents), int(act_seqs.shape[1]), int(act_seqs.shape[0]), float(gamma),
                world.pos_x.data_ptr(), world.pos_y.data_ptr(), world.vel_x.data_ptr(), world.vel_y.data_ptr(),
                self.ideal_shape.data_ptr(), self.ideal_vel.data_ptr(), world.step_count.data_ptr(), act_seqs.data_ptr(),
                out["ret"].data_ptr(), _native.ptr(out.get("indiv")), _native.ptr(out.get("steps")),
                _native.current_stream(world.device))
        return _native.bind_launch(lib.fg_rollout_hd_returns, p, *args, keep=(act_seqs, out))

    def bind_rollout_returns_sampled(self, world, mean, candidates, out, gamma=1.0):
        """`bind_rollout_returns` with the candidates drawn inside the launch (`fg_rollout_hd_returns_sampled`): candidate c's
        action at step k is clamp(mean[k] + sigma eps) with eps from the planner's counter stream, so no [C,K,B,N,2] tensor
        exists.  mean [K,B,N,2] fp32 contiguous is read in place; `out` as for `bind_rollout_returns`.  Returns
        `launch(noise_offset, sigma, clip)`: the planner's scalars as they are at the call.  The launch reads the world's state
        and writes only `out`; the env's RNG offset is neither read nor moved."""
        lib = _native.load()
        p = self.params(world)
        head = (world.num_envs, len(world.agents), int(mean.shape[0]), int(candidates), float(gamma))
        tail = (world.pos_x.data_ptr(), world.pos_y.data_ptr(), world.vel_x.data_ptr(), world.vel_y.data_ptr(),
                self.ideal_shape.data_ptr(), self.ideal_vel.data_ptr(), world.step_count.data_ptr(), mean.data_ptr(),
                out["ret"].data_ptr(), _native.ptr(out.get("indiv")), _native.ptr(out.get("steps")),
                _native.current_stream(world.device))
        keep = (mean, out)

        def launch(noise_offset, sigma, clip):
            rc = lib.fg_rollout_hd_returns_sampled(p, *head, int(noise_offset), float(sigma), float(clip), *tail)
            if rc:
                _native.check(rc)
            return keep
        return launch

    def bind_rollout_returns_sampled_std(self, world, mean, std, candidates, out):
        """`bind_rollout_returns_sampled` with a sigma per element (`fg_rollout_hd_returns_sampled_std`): std [K,B,N,2] fp32
        contiguous, finite and >= 0, read in place beside `mean`.  Returns `launch(noise_offset, gamma, clip)`."""
        lib = _native.load()
        p = self.params(world)
        head = (world.num_envs, len(world.agents), int(mean.shape[0]), int(candidates))
        tail = (world.pos_x.data_ptr(), world.pos_y.data_ptr(), world.vel_x.data_ptr(), world.vel_y.data_ptr(),
                self.ideal_shape.data_ptr(), self.ideal_vel.data_ptr(), world.step_count.data_ptr(), mean.data_ptr(),
                std.data_ptr(), out["ret"].data_ptr(), _native.ptr(out.get("indiv")), _native.ptr(out.get("steps")),
                _native.current_stream(world.device))
        keep = (mean, std, out)

        def launch(noise_offset, gamma, clip):
            rc = lib.fg_rollout_hd_returns_sampled_std(p, *head, float(gamma), int(noise_offset), float(clip), *tail)
            if rc:
                _native.check(rc)
            return keep
        return launch

    def upload_mt_streams(self, world):
        """Copy every env's legacy MT19937 state (RandomState(seed + 1000 b), at its CURRENT
        position) to the device; from here on `reset_mt` continues those streams on the GPU."""
        B = world.num_envs
        st = np.zeros((B, 626), dtype=np.uint32)
        for b, rs in enumerate(self._streams(B)):
            _, key, pos = rs.get_state()[:3]
            st[b, :624] = key
            st[b, 624] = pos
        self._mt_state = torch.as_tensor(st.view(np.int32)).to(world.device)
        return self._mt_state

    def reset_mt(self, world, mask=None):
        """Scenario.reset_world on the GPU from the reference's own RNG streams (bit-exact with
        the host path `reset_world`): masked envs draw N agent positions, N landmark positions
        and the ideal velocity from their MT19937 state, which advances in place."""
        if getattr(self, "_mt_state", None) is None or self._mt_state.shape[0] != world.num_envs:
            self.upload_mt_streams(world)
        lib = _native.load()
        _native.check(lib.fg_reset_hd_mt(
            world.num_envs, len(world.agents), _native.ptr(mask), self._mt_state.data_ptr(),
            world.pos_x.data_ptr(), world.pos_y.data_ptr(), world.vel_x.data_ptr(), world.vel_y.data_ptr(),
            self.ideal_shape.data_ptr(), self.ideal_vel.data_ptr(), world.landmark_pos.data_ptr(),
            world.step_count.data_ptr(), _native.current_stream(world.device)))
        self._cache = None

    def reset_mt_done(self, world, obs=None):
        """The vec-env worker's `if all(done): ob = env.reset()` (env_wrappers.py:14-18) for every env at once, decided on
        the device (`fg_reset_hd_mt_done`): envs whose step counter has reached world_length restart from their own
        MT19937 streams and, with `obs` [B, N, 6N], get their reset observation written over the step's."""
        if getattr(self, "_mt_state", None) is None or self._mt_state.shape[0] != world.num_envs:
            self.upload_mt_streams(world)
        _native.check(_native.load().fg_reset_hd_mt_done(
            world.num_envs, len(world.agents), int(world.world_length), self._mt_state.data_ptr(),
            world.pos_x.data_ptr(), world.pos_y.data_ptr(), world.vel_x.data_ptr(), world.vel_y.data_ptr(),
            self.ideal_shape.data_ptr(), self.ideal_vel.data_ptr(), world.landmark_pos.data_ptr(),
            world.step_count.data_ptr(), _native.ptr(obs), self.obs_env_pitch(obs, len(world.agents)),
            _native.current_stream(world.device)))
        self._cache = None

    def bind_reset_mt_done(self, world, obs=None):
        """`reset_mt_done` with every pointer resolved once: returns `launch()`, one ctypes call per vec-env step."""
        if getattr(self, "_mt_state", None) is None or self._mt_state.shape[0] != world.num_envs:
            self.upload_mt_streams(world)
        fn = _native.load().fg_reset_hd_mt_done
        args = (world.num_envs, len(world.agents), int(world.world_length), self._mt_state.data_ptr(),
                world.pos_x.data_ptr(), world.pos_y.data_ptr(), world.vel_x.data_ptr(), world.vel_y.data_ptr(),
                self.ideal_shape.data_ptr(), self.ideal_vel.data_ptr(), world.landmark_pos.data_ptr(),
                world.step_count.data_ptr(), _native.ptr(obs), self.obs_env_pitch(obs, len(world.agents)),
                _native.current_stream(world.device))
        keep = (self._mt_state, obs)

        def launch():
            rc = fn(*args)
            if rc:
                _native.check(rc)
            self._cache = None
            return keep
        return launch

    def reset_device(self, world, mask=None, rng_offset=0):
        """Throughput-mode reset on the GPU (counter RNG, distributional parity only)."""
        lib = _native.load()
        _native.check(lib.fg_reset_hd(
            self.params(world, rng_offset=rng_offset), world.num_envs, len(world.agents), _native.ptr(mask),
            world.pos_x.data_ptr(), world.pos_y.data_ptr(), world.vel_x.data_ptr(), world.vel_y.data_ptr(),
            self.ideal_shape.data_ptr(), self.ideal_vel.data_ptr(), world.step_count.data_ptr(),
            _native.current_stream(world.device)))
        self._cache = None

    # ---- per-agent callbacks (reference signature) -----------------------------
    def _fresh(self, world):
        if self._cache is None:
            B, N = world.num_envs, len(world.agents)
            f = dict(dtype=torch.float32, device=world.device)
            out = dict(obs=torch.empty((B, N, 6 * N), **f), reward=torch.empty((B, N), **f),
                       indiv=torch.empty((B, N), **f))
            self.observe_batch(world, out)
        return self._cache

    def observation(self, agent, world):
        """:38-59 for `agent` in every env -> [B, 6N].  Also applies the
        reference's side effect of re-centring the landmarks on the agents (:40-44)."""
        out = self._fresh(world)
        cen = torch.stack((world.pos_x.mean(1), world.pos_y.mean(1)), -1) - world.landmark_pos.mean(1)
        world.landmark_pos += cen[:, None, :]
        return out["obs"][:, agent.i]

    def reward(self, agent, world):
        """:61-75 individual reward of `agent` in every env -> [B]."""
        return self._fresh(world)["indiv"][:, agent.i]

    def benchmark_data(self, agent, world):
        """:97-117 for `agent` in every env -> dict of [B] tensors.  The env shell evaluates it right after
        `observation` (environment.py:127-131), which has just re-centred the landmarks on the agents (:40-44):
        the landmark positions it measures against are ideal_shape + centroid(agents)."""
        rew = self.reward(agent, world)
        pos, _ = world.get_state()
        d = (pos - pos[:, agent.i:agent.i + 1]).norm(dim=-1)
        a0 = world.agents[0]
        collisions = (d < (a0.size + a0.size) / 2).sum(1)       # is_collision (:119-121), `agent` itself included (:101-104)
        lm = self.ideal_shape + pos.mean(1, keepdim=True)
        dl = (pos[:, :, None, :] - lm[:, None, :, :]).norm(dim=-1).min(1).values     # per landmark: its nearest agent
        return {'reward': rew, 'collisions': collisions, 'min_dists': dl.sum(1),
                'occupied_landmarks': (dl < 0.1).sum(1)}

    def is_collision(self, agent1, agent2):
        """:119-121 -> bool [B]."""
        dist = (agent1.state.p_pos - agent2.state.p_pos).norm(dim=-1)
        return dist < (agent1.size + agent2.size) / 2

    def generate_shape(self, layer, layer_shapes=None):
        """:123-139 default hierarchical target shape, [3, ..., 3, 2] nested like the reference."""
        table = np.array([
            [[0, -1], [0.5, 0], [0, 1]],
            [[0, 1.6], [-1, 0], [1, 0]],
            [[1.5, 0], [0, 0], [-1.5, 0]],
            [[0, 0.6], [1, 0], [-1, 0]],
        ]) if layer_shapes is None else np.asarray(layer_shapes)
        assert layer < table.shape[0], 'Layer shape is not enough!'
        if layer == 0:
            return table[0]
        inner = self.generate_shape(layer - 1, layer_shapes)
        return np.array([table[layer][i] + inner * 0.45 for i in range(table.shape[1])])
