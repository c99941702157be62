"""C-ABI checks that need no GPU: the library builds and loads, exports every
symbol include/formation_hip.h declares, the ctypes mirror of FgParams has the
C layout, and argument validation returns the documented status codes before
any launch.  Also: the product path fails loudly without a GPU / library."""
import ctypes
import os
import re

import numpy as np
import pytest

from formation_gym import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "formation_hip.h")


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def _declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fg_[a-z_0-9]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    names = _declared_symbols()
    assert len(names) >= 10
    for n in names:
        assert hasattr(lib, n), "library does not export %s" % n
        assert n in _native.SIGNATURES, "ctypes binding lacks %s" % n
    assert sorted(_native.SIGNATURES) == names


def test_abi_version_and_struct_layout(lib, tmp_path):
    """The ctypes mirrors must have the C layout: compile the header with gcc and compare
    sizeof / offsetof of every field."""
    import subprocess
    assert lib.fg_abi_version() == _native.ABI_VERSION == 8
    assert "#define FG_ABI_VERSION 8" in open(HEADER).read()
    structs = {"FgParams": _native.FgParams, "FgScenario": _native.FgScenario, "FgWall": _native.FgWall}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "formation_hip.h"', 'int main(void){']
    for name, cls in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for fname, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, fname, name, fname))
    lines.append('return 0;}')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, cls in structs.items():
        assert int(got[name]) == ctypes.sizeof(cls), name
        for fname, _ in cls._fields_:
            assert int(got["%s.%s" % (name, fname)]) == getattr(cls, fname).offset, (name, fname)
    assert _native.MAX_WALLS == 4 and "#define FG_MAX_WALLS 4" in open(HEADER).read()
    assert _native.AGENT_PROPS == 8 and "#define FG_AGENT_PROPS 8" in open(HEADER).read()


def test_algorithmic_bytes_and_geometry(lib):
    for n, want in [(9, 2437), (27, 18943), (81, 161773), (243, 1430071)]:
        assert _native.step_hd_bytes(n) == want == 24 * n * n + 53 * n + 16
    for n in (3, 4, 9, 10, 27, 64, 65, 81, 243, 1024):
        cfg = _native.kernel_config(n)
        assert cfg["threads"] % 64 == 0 and cfg["threads"] <= 1024 and cfg["envs_per_wg"] >= 1
        assert cfg["lds_bytes"] <= 160 * 1024
    with pytest.raises(_native.FormationHipError) as e:
        _native.kernel_config(1025)
    assert e.value.code == _native.FG_ERR_UNSUPPORTED_N


def _params(**kw):
    d = dict(dt=0.1, damping=0.25, contact_force=100.0, contact_margin=1e-3, sensitivity=5.0, mass=1.0,
             dist_min=0.06, collide_thresh=0.03, world_length=100, auto_reset=0, seed=0, rng_offset=0,
             accel=0.0, max_speed=0.0, u_noise=0.0, num_walls=0)
    d.update(kw)
    return _native.FgParams(**d)


def test_argument_validation_before_any_launch(lib):
    buf = np.zeros(4096, dtype=np.float32)
    p = buf.ctypes.data          # host pointer: validation must reject before it is ever used
    P = _params()
    ok_ptrs = [p] * 16
    assert lib.fg_step_hd(P, -1, 9, *ok_ptrs) == _native.FG_ERR_BAD_ARG                # B < 0
    assert b"B must be" in lib.fg_last_error()
    # an empty batch (B = 0), zero steps (K = 0) and zero agents to decode are successful no-ops, NULL buffers allowed
    assert lib.fg_step_hd(P, 0, 9, *([None] * 16)) == _native.FG_OK
    assert lib.fg_physics_step(P, 0, 9, *([None] * 6)) == _native.FG_OK
    assert lib.fg_rollout_hd(P, 0, 9, 5, *([None] * 12), 1, None) == _native.FG_OK
    assert lib.fg_rollout_hd(P, 4, 9, 0, *([None] * 12), 1, None) == _native.FG_OK
    assert lib.fg_reset_hd(P, 0, 9, *([None] * 9)) == _native.FG_OK
    assert lib.fg_decode_actions(_native.FG_ACT_INDEX, 0, None, None, None) == _native.FG_OK
    assert lib.fg_step_hd(P, 4, 2, *ok_ptrs) == _native.FG_ERR_UNSUPPORTED_N           # obs needs N >= 3
    assert lib.fg_step_hd(P, 4, 2000, *ok_ptrs) == _native.FG_ERR_UNSUPPORTED_N
    null_obs = list(ok_ptrs); null_obs[8] = None
    assert lib.fg_step_hd(P, 4, 9, *null_obs) == _native.FG_ERR_BAD_ARG                # required pointer
    mis = list(ok_ptrs); mis[8] = p + 4
    assert lib.fg_step_hd(P, 4, 9, *mis) == _native.FG_ERR_ALIGNMENT                   # obs 16-byte aligned
    assert b"aligned" in lib.fg_last_error()
    assert lib.fg_step_hd(None, 4, 9, *ok_ptrs) == _native.FG_ERR_BAD_ARG
    assert lib.fg_step_hd(_params(mass=0.0), 4, 9, *ok_ptrs) == _native.FG_ERR_BAD_ARG
    assert lib.fg_step_hd(_params(num_walls=5), 4, 9, *ok_ptrs) == _native.FG_ERR_BAD_ARG
    assert lib.fg_step_hd(_params(max_speed=-1.0), 4, 9, *ok_ptrs) == _native.FG_ERR_BAD_ARG
    assert lib.fg_physics_step(P, 4, 1, *([p] * 6)) == _native.FG_ERR_UNSUPPORTED_N
    assert lib.fg_observe_hd(P, 4, 9, p, p, p, p, p, p, p, None, None, None, None, None, None, None, None) \
        == _native.FG_ERR_BAD_ARG                                                      # nothing to write
    assert lib.fg_rollout_hd(P, 4, 9, -1, *([p] * 12), 1, None) == _native.FG_ERR_BAD_ARG   # K < 0
    assert lib.fg_reset_hd(P, 4, 5000, *([p] * 9)) == _native.FG_ERR_UNSUPPORTED_N
    assert lib.fg_step_basic(P, 4, 1100, 3, 1, *([p] * 13)) == _native.FG_ERR_UNSUPPORTED_N
    sc = _native.FgScenario(kind=_native.FG_SCN_OBSTACLE, num_landmarks=4, num_obstacles=3, penalty=2.0)
    assert lib.fg_step_scenario(P, sc, 4, 1022, 1, *([p] * 14)) == _native.FG_ERR_UNSUPPORTED_N   # N + M > 1024
    assert lib.fg_step_scenario(P, _native.FgScenario(kind=9, num_landmarks=4), 4, 4, 1, *([p] * 14)) == _native.FG_ERR_BAD_ARG
    assert lib.fg_step_scenario(P, None, 4, 4, 1, *([p] * 14)) == _native.FG_ERR_BAD_ARG
    assert lib.fg_rollout_scenario(P, sc, 4, 4, 0, *([None] * 14), 1, None) == _native.FG_OK     # K = 0: no-op
    assert lib.fg_rollout_scenario(P, sc, 4, 4, -2, *([p] * 14), 1, None) == _native.FG_ERR_BAD_ARG
    assert lib.fg_rollout_scenario(P, sc, 4, 1022, 3, *([p] * 14), 1, None) == _native.FG_ERR_UNSUPPORTED_N
    assert lib.fg_reset_scenario(P, sc, 0, 4, *([None] * 10)) == _native.FG_OK          # empty batch
    assert lib.fg_reset_scenario(P, None, 4, 4, *([p] * 10)) == _native.FG_ERR_BAD_ARG
    assert lib.fg_reset_scenario(P, sc, 4, 1022, *([p] * 10)) == _native.FG_ERR_UNSUPPORTED_N
    assert lib.fg_reset_scenario(P, sc, 4, 4, None, p, p, p, p, p, None, None, p, None) == _native.FG_ERR_BAD_ARG   # obstacles missing
    assert lib.fg_reset_scenario(P, sc, 4, 4, None, p, p, p, p, p + 4, p, p, p, None) == _native.FG_ERR_ALIGNMENT
    assert lib.fg_decode_actions(0, 12, p, p, None) == _native.FG_ERR_BAD_ARG           # unknown mode
    assert lib.fg_decode_actions(_native.FG_ACT_INDEX, -3, p, p, None) == _native.FG_ERR_BAD_ARG
    assert lib.fg_decode_actions(_native.FG_ACT_ONEHOT5, 12, None, p, None) == _native.FG_ERR_BAD_ARG
    assert lib.fg_decode_actions(_native.FG_ACT_ARGMAX, 12, p + 4, p, None) == _native.FG_ERR_ALIGNMENT
    # per-agent table / communication state pointers are checked for alignment; the landmark-scenario entry points take
    # the table (ABI 7) and refuse the communication state instead of ignoring it
    assert lib.fg_step_hd(_params(agent_props=p + 2), 4, 9, *ok_ptrs) == _native.FG_ERR_ALIGNMENT
    assert lib.fg_step_hd(_params(comm_state=p + 4), 4, 9, *ok_ptrs) == _native.FG_ERR_ALIGNMENT
    assert lib.fg_step_hd(_params(dist_min=0.0), 4, 9, *ok_ptrs) == _native.FG_ERR_BAD_ARG
    assert lib.fg_step_basic(_params(comm_state=p), 4, 3, 3, 1, *([p] * 13)) == _native.FG_ERR_BAD_ARG
    assert b"formation_hd_env entry points only" in lib.fg_last_error()
    assert lib.fg_update_comm(P, 0, 9, None, None, None) == _native.FG_OK
    assert lib.fg_update_comm(P, 4, 9, None, p, None) == _native.FG_ERR_BAD_ARG
    assert lib.fg_update_comm(P, 4, 9, p + 4, p, None) == _native.FG_ERR_ALIGNMENT
    assert lib.fg_update_comm(P, 4, 5000, p, p, None) == _native.FG_ERR_UNSUPPORTED_N
    # device-decided MT19937 reset: needs the step counters and an episode length
    assert lib.fg_reset_hd_mt_done(0, 9, 100, *([None] * 10), 0, None) == _native.FG_OK
    assert lib.fg_reset_hd_mt_done(4, 9, 0, *([p] * 10), 0, None) == _native.FG_ERR_BAD_ARG
    assert lib.fg_reset_hd_mt_done(4, 9, 100, *([p] * 9), p, 7, None) == _native.FG_ERR_BAD_ARG        # odd / short env pitch
    assert lib.fg_reset_hd_mt_done(4, 9, 100, *([p] * 9), p + 4, 0, None) == _native.FG_ERR_ALIGNMENT
    # arenas: argument checks (creating one needs a device)
    h, b = ctypes.c_void_p(), ctypes.c_void_p()
    assert lib.fg_arena_create(0, 0, 0, ctypes.byref(h), None, None) == _native.FG_ERR_BAD_ARG
    assert lib.fg_arena_create(0, 1 << 20, 0, None, None, None) == _native.FG_ERR_BAD_ARG
    assert lib.fg_arena_map(None, None, 0, ctypes.byref(b)) == _native.FG_ERR_BAD_ARG
    assert lib.fg_arena_unmap(None, None) == _native.FG_ERR_BAD_ARG
    assert lib.fg_arena_trim(None) == _native.FG_ERR_BAD_ARG
    assert lib.fg_arena_destroy(None) == _native.FG_OK
    # fg_policy_bfs: N must be per_layer^L, 2 <= per_layer <= 8
    assert lib.fg_policy_bfs(0, 9, 3, None, 0, None, None) == _native.FG_OK
    assert lib.fg_policy_bfs(4, 10, 3, p, 0, p, None) == _native.FG_ERR_UNSUPPORTED_N
    assert b"per_layer" in lib.fg_last_error()
    assert lib.fg_policy_bfs(4, 81, 9, p, 0, p, None) == _native.FG_ERR_UNSUPPORTED_N     # per_layer > 8
    assert lib.fg_policy_bfs(4, 9, 3, None, 0, p, None) == _native.FG_ERR_BAD_ARG
    assert lib.fg_policy_bfs(4, 9, 3, p, 7, p, None) == _native.FG_ERR_BAD_ARG            # odd / short env stride
    assert lib.fg_policy_bfs(4, 9, 3, p + 4, 0, p, None) == _native.FG_ERR_ALIGNMENT
    assert lib.fg_policy_bfs(-1, 9, 3, p, 0, p, None) == _native.FG_ERR_BAD_ARG
    with pytest.raises(_native.FormationHipError):
        _native.check(lib.fg_step_hd(P, -1, 9, *ok_ptrs))


# ---- every non-actor entry point that checks arguments: status and fg_last_error() of each failing check, and their order ----
# An entry's arguments in C order.  A bare name is a stand-in pointer (address 4096: aligned for everything, never dereferenced
# before a launch), NAME=V an integer or None, `params` / `scenario` / `actor` a struct built from keyword arguments (None: NULL),
# `out` a 512-byte text buffer followed by its length, `plan` a void** to receive a plan.
_STATE = "pos_x pos_y vel_x vel_y "
_HD_OUT = "obs reward indiv done "
_SCN_STATE = _STATE + "act landmarks obst_pos obst_vel step " + _HD_OUT
CABI_ENTRIES = {
    "fg_step_hd": "params B=4 N=9 " + _STATE + "act ideal_shape ideal_vel step " + _HD_OUT + "near_lm near_ag hd_idx stream=None",
    "fg_step_hd_plan": "params B=4 N=9 " + _STATE + "act ideal_shape ideal_vel step " + _HD_OUT
                       + "near_lm near_ag hd_idx stream=None plan",
    "fg_physics_step": "params B=4 N=9 " + _STATE + "act stream=None",
    "fg_observe_hd": "params B=4 N=9 " + _STATE + "ideal_shape ideal_vel step " + _HD_OUT + "near_lm near_ag hd_idx stream=None",
    "fg_rollout_hd": "params B=4 N=9 K=5 " + _STATE + "act ideal_shape ideal_vel step " + _HD_OUT + "obs_every=1 stream=None",
    "fg_rollout_hd_policy": "params B=4 N=9 K=5 per=3 " + _STATE + "act ideal_shape ideal_vel step " + _HD_OUT
                            + "obs_every=1 stream=None",
    "fg_reset_hd": "params B=4 N=9 mask " + _STATE + "ideal_shape ideal_vel step stream=None",
    "fg_reset_hd_mt": "B=4 N=9 mask mt_state " + _STATE + "ideal_shape ideal_vel landmark_pos step stream=None",
    "fg_reset_hd_mt_done": "B=4 N=9 world_length=100 mt_state " + _STATE + "ideal_shape ideal_vel landmark_pos step obs "
                           "obs_env_pitch=0 stream=None",
    "fg_reset_scenario": "params scenario B=4 N=4 mask " + _STATE + "landmarks obst_pos obst_vel step stream=None",
    "fg_reset_scenario_mt": "scenario B=4 N=4 mask world_length=100 mt_state " + _STATE + "landmarks obst_pos obst_vel step "
                            "stream=None",
    "fg_step_scenario": "params scenario B=4 N=4 do_physics=1 " + _SCN_STATE + "stream=None",
    "fg_step_basic": "params B=4 N=3 L=3 do_physics=1 " + _STATE + "act landmarks step " + _HD_OUT + "near_ag stream=None",
    "fg_rollout_scenario": "params scenario B=4 N=4 K=5 " + _SCN_STATE + "near_ag obs_every=1 stream=None",
    "fg_update_comm": "params B=4 N=9 action_c comm_state stream=None",
    "fg_update_comm_dim": "params B=4 N=9 dim_c=3 action_c comm_state stream=None",
    "fg_policy_bfs": "B=4 N=9 per=3 obs obs_env_stride=0 act stream=None",
    "fg_policy_bfs_state": "B=4 N=9 per=3 pos_x pos_y ideal_shape ideal_vel act stream=None",
    "fg_decode_actions": "mode=%d count=12 action u_out stream=None" % _native.FG_ACT_ARGMAX,
    "fg_actor_noise": "params B=4 N=9 eps stream=None",
    "fg_kernel_config": "N=9 threads=None envs_per_wg=None lds_bytes=None",
    "fg_describe_launch": "params scenario=None B=4 N=9 K=5 per=0 obs_every=1 index_outputs=0 out",
    "fg_rollout_scenario_actor": "params scenario actor log_std B=4 N=4 K=5 " + _STATE + "landmarks obst_pos obst_vel step "
                                 + _HD_OUT + "act_out logp obs_every=1 stream=None",
    "fg_describe_scenario_actor_launch": "params scenario actor log_std B=4 N=4 K=5 obs_every=1 out",
}
_OBSTACLE = dict(kind=_native.FG_SCN_OBSTACLE, num_landmarks=4, num_obstacles=3, penalty=2.0)     # N = 4: a reference shape
_ACTOR = dict(hidden=64, out_tanh=1, w1=4096, b1=4096, w2=4096, b2=4096, w3=4096, b3=4096)


_STRUCTS = {"params": (_params, {}), "scenario": (_native.FgScenario, _OBSTACLE), "actor": (_native.FgActor, _ACTOR)}


def _cabi_call(lib, entry, **wrong):
    """(status, fg_last_error()) of `entry` with CABI_ENTRIES' arguments, `wrong` replacing some by name: a struct's value is
    None or keyword arguments that update its defaults, `out=None` passes no text buffer."""
    names = [tok.partition("=")[0] for tok in CABI_ENTRIES[entry].split()]
    assert set(wrong) <= set(names), (entry, wrong)
    args = []
    for tok in CABI_ENTRIES[entry].split():
        name, _, default = tok.partition("=")
        value = wrong[name] if name in wrong else eval(default) if default else {} if name in _STRUCTS else 4096
        if name in _STRUCTS and value is not None:
            make, base = _STRUCTS[name]
            value = make(**dict(base, **value))
        elif name == "out":
            args.append(ctypes.create_string_buffer(512) if value is not None else None)
            value = 512
        elif name == "plan" and value is not None:
            value = ctypes.pointer(ctypes.c_void_p())
        args.append(value)
    rc = getattr(lib, entry)(*args)
    return rc, lib.fg_last_error().decode()


# (entry, what is wrong with the call, status, fg_last_error()); a text of None: the call succeeds without a launch (an empty
# batch, zero steps).  The literals are the answers of the library before the entries shared one call builder and one launcher.
CABI_BAD_CALLS = [
    ('fg_step_hd', dict(params=None), -1, 'params is NULL'),
    ('fg_step_hd_plan', dict(params=None), -1, 'params is NULL'),
    ('fg_physics_step', dict(params=None), -1, 'params is NULL'),
    ('fg_observe_hd', dict(params=None), -1, 'params is NULL'),
    ('fg_rollout_hd', dict(params=None), -1, 'params is NULL'),
    ('fg_rollout_hd_policy', dict(params=None), -1, 'params is NULL'),
    ('fg_reset_hd', dict(params=None), -1, 'params is NULL'),
    ('fg_reset_scenario', dict(params=None), -1, 'params is NULL'),
    ('fg_step_scenario', dict(params=None), -1, 'params is NULL'),
    ('fg_step_basic', dict(params=None), -1, 'params is NULL'),
    ('fg_rollout_scenario', dict(params=None), -1, 'params is NULL'),
    ('fg_update_comm', dict(params=None), -1, 'params is NULL'),
    ('fg_update_comm_dim', dict(params=None), -1, 'params is NULL'),
    ('fg_actor_noise', dict(params=None), -1, 'params is NULL'),
    ('fg_describe_launch', dict(params=None), -1, 'params is NULL'),
    ('fg_rollout_scenario_actor', dict(params=None), -1, 'params is NULL'),
    ('fg_describe_scenario_actor_launch', dict(params=None), -1, 'params is NULL'),
    ('fg_step_hd', dict(params={'mass': 0.0}), -1, 'params: mass, contact_margin and dt must be > 0'),
    ('fg_step_hd', dict(params={'num_walls': 5}), -1, 'params: 0 <= num_walls <= 4, accel/max_speed/u_noise >= 0'),
    ('fg_step_hd', dict(params={'dist_min': 0.0}), -1, 'params: dist_min must be > 0'),
    ('fg_step_hd', dict(params={'agent_props': 4098}), -3, 'params: agent_props must be 4-byte, comm_state 8-byte aligned'),
    ('fg_step_hd', dict(params={'comm_state': 4100}), -3, 'params: agent_props must be 4-byte, comm_state 8-byte aligned'),
    ('fg_step_hd', dict(params={'mass': 0.0, 'dist_min': 0.0, 'comm_state': 4100}), -1, 'params: mass, contact_margin and dt must be > 0'),
    ('fg_step_hd', dict(params={'mass': 0.0}, B=-1, N=2, obs=None, act=4100), -1, 'params: mass, contact_margin and dt must be > 0'),
    ('fg_rollout_hd', dict(params=None, B=-1, N=2, K=-1, pos_x=None, obs=4100), -1, 'params is NULL'),
    ('fg_rollout_scenario', dict(params={'dt': 0.0}, scenario=None, B=-1, N=1, K=-1), -1, 'params: mass, contact_margin and dt must be > 0'),
    ('fg_step_hd', dict(B=-1), -1, 'B must be >= 0'),
    ('fg_step_hd', dict(N=2), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_step_hd', dict(N=1025), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_step_hd', dict(B=0, N=2), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_step_hd', dict(B=-1, N=2), -1, 'B must be >= 0'),
    ('fg_step_hd', dict(obs=None), -1, 'fg_step_hd: a required pointer is NULL'),
    ('fg_step_hd', dict(step=None), -1, 'fg_step_hd: a required pointer is NULL'),
    ('fg_step_hd', dict(reward=None), -1, 'fg_step_hd: a required pointer is NULL'),
    ('fg_step_hd', dict(obs=4100), -3, 'obs must be 16-byte, act/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_step_hd', dict(act=4100), -3, 'obs must be 16-byte, act/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_step_hd', dict(ideal_vel=4100), -3, 'obs must be 16-byte, act/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_step_hd', dict(pos_x=None, obs=4100), -1, 'fg_step_hd: a required pointer is NULL'),
    ('fg_step_hd', dict(N=2, obs=None), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_step_hd', dict(params={'obs_env_pitch': 7}), -1, 'params: obs_env_pitch must be 0 or an even number of floats >= 6 N^2'),
    ('fg_step_hd', dict(params={'obs_env_pitch': 484}), -1, 'params: obs_env_pitch must be 0 or an even number of floats >= 6 N^2'),
    ('fg_step_hd', dict(params={'obs_env_pitch': 7}, obs=4100), -3, 'obs must be 16-byte, act/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_step_hd', dict(B=0, obs=4100, pos_x=None), -3, 'obs must be 16-byte, act/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_step_hd_plan', dict(B=-1), -1, 'B must be >= 0'),
    ('fg_step_hd_plan', dict(N=2), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_step_hd_plan', dict(N=1025), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_step_hd_plan', dict(B=0, N=2), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_step_hd_plan', dict(B=-1, N=2), -1, 'B must be >= 0'),
    ('fg_step_hd_plan', dict(obs=None), -1, 'fg_step_hd: a required pointer is NULL'),
    ('fg_step_hd_plan', dict(step=None), -1, 'fg_step_hd: a required pointer is NULL'),
    ('fg_step_hd_plan', dict(reward=None), -1, 'fg_step_hd: a required pointer is NULL'),
    ('fg_step_hd_plan', dict(obs=4100), -3, 'obs must be 16-byte, act/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_step_hd_plan', dict(act=4100), -3, 'obs must be 16-byte, act/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_step_hd_plan', dict(ideal_vel=4100), -3, 'obs must be 16-byte, act/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_step_hd_plan', dict(pos_x=None, obs=4100), -1, 'fg_step_hd: a required pointer is NULL'),
    ('fg_step_hd_plan', dict(N=2, obs=None), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_step_hd_plan', dict(params={'obs_env_pitch': 7}), -1, 'params: obs_env_pitch must be 0 or an even number of floats >= 6 N^2'),
    ('fg_step_hd_plan', dict(params={'obs_env_pitch': 484}), -1, 'params: obs_env_pitch must be 0 or an even number of floats >= 6 N^2'),
    ('fg_step_hd_plan', dict(params={'obs_env_pitch': 7}, obs=4100), -3, 'obs must be 16-byte, act/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_step_hd_plan', dict(B=0, obs=4100, pos_x=None), -3, 'obs must be 16-byte, act/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_step_hd', dict(B=0, pos_x=None, obs=None), 0, None),
    ('fg_step_hd_plan', dict(plan=None), -1, 'fg_step_hd_plan: plan is NULL'),
    ('fg_step_hd_plan', dict(plan=None, params=None, B=-1), -1, 'fg_step_hd_plan: plan is NULL'),
    ('fg_physics_step', dict(B=0, N=1, pos_x=None), 0, None),
    ('fg_physics_step', dict(B=-1, N=1), -1, 'B must be >= 0'),
    ('fg_physics_step', dict(N=1), -2, 'N must be in [2, 1024]'),
    ('fg_physics_step', dict(N=1025), -2, 'N must be in [2, 1024]'),
    ('fg_physics_step', dict(vel_y=None), -1, 'fg_physics_step: a required pointer is NULL'),
    ('fg_physics_step', dict(act=None), -1, 'fg_physics_step: a required pointer is NULL'),
    ('fg_physics_step', dict(act=4100), -3, 'act must be 8-byte aligned'),
    ('fg_physics_step', dict(pos_x=None, act=4100), -1, 'fg_physics_step: a required pointer is NULL'),
    ('fg_physics_step', dict(N=1, act=None), -2, 'N must be in [2, 1024]'),
    ('fg_physics_step', dict(params={'obs_env_pitch': 7}), -1, 'params: obs_env_pitch must be 0 or an even number of floats >= 6 N^2'),
    ('fg_physics_step', dict(params={'obs_env_pitch': 7}, act=4100), -3, 'act must be 8-byte aligned'),
    ('fg_observe_hd', dict(B=0, N=2, pos_x=None), 0, None),
    ('fg_observe_hd', dict(B=-1, N=2), -1, 'B must be >= 0'),
    ('fg_observe_hd', dict(N=2), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_observe_hd', dict(N=1025), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_observe_hd', dict(ideal_vel=None), -1, 'fg_observe_hd: a required pointer is NULL'),
    ('fg_observe_hd', dict(obs=None, reward=None), -1, 'fg_observe_hd: obs and reward both NULL'),
    ('fg_observe_hd', dict(pos_x=None, obs=None, reward=None), -1, 'fg_observe_hd: a required pointer is NULL'),
    ('fg_observe_hd', dict(obs=4100), -3, 'obs must be 16-byte, ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_observe_hd', dict(ideal_shape=4100), -3, 'obs must be 16-byte, ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_observe_hd', dict(obs=4100, reward=None), -3, 'obs must be 16-byte, ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_observe_hd', dict(obs=None, reward=None, ideal_shape=4100), -1, 'fg_observe_hd: obs and reward both NULL'),
    ('fg_observe_hd', dict(params={'obs_env_pitch': 7}), -1, 'params: obs_env_pitch must be 0 or an even number of floats >= 6 N^2'),
    ('fg_observe_hd', dict(params={'obs_env_pitch': 7}, obs=4100), -3, 'obs must be 16-byte, ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_observe_hd', dict(N=2, pos_x=None), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_rollout_hd', dict(B=0, N=2, pos_x=None), 0, None),
    ('fg_rollout_hd', dict(K=0, N=2, pos_x=None), 0, None),
    ('fg_rollout_hd', dict(B=-1, K=0), 0, None),
    ('fg_rollout_hd', dict(B=0, K=-1), 0, None),
    ('fg_rollout_hd', dict(B=-1), -1, 'B and K must be >= 0'),
    ('fg_rollout_hd', dict(K=-1), -1, 'B and K must be >= 0'),
    ('fg_rollout_hd', dict(B=-1, N=2), -1, 'B and K must be >= 0'),
    ('fg_rollout_hd', dict(N=2), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_rollout_hd', dict(N=1025), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_rollout_hd', dict(pos_x=None), -1, 'fg_rollout_hd: a required pointer is NULL'),
    ('fg_rollout_hd', dict(reward=None), -1, 'fg_rollout_hd: a required pointer is NULL'),
    ('fg_rollout_hd', dict(step=None), -1, 'fg_rollout_hd: a required pointer is NULL'),
    ('fg_rollout_hd', dict(obs=None, reward=None), -1, 'fg_rollout_hd: a required pointer is NULL'),
    ('fg_rollout_hd', dict(obs=4100), -3, 'obs_seq must be 16-byte, act_seq/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_rollout_hd', dict(act=4100), -3, 'obs_seq must be 16-byte, act_seq/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_rollout_hd', dict(ideal_shape=4100), -3, 'obs_seq must be 16-byte, act_seq/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_rollout_hd', dict(reward=None, obs=4100), -1, 'fg_rollout_hd: a required pointer is NULL'),
    ('fg_rollout_hd', dict(N=2, reward=None), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_rollout_hd', dict(params={'obs_env_pitch': 7}), -1, 'params: obs_env_pitch must be 0 or an even number of floats >= 6 N^2'),
    ('fg_rollout_hd', dict(params={'obs_env_pitch': 7}, obs=4100), -3, 'obs_seq must be 16-byte, act_seq/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_rollout_hd_policy', dict(B=0, N=2, pos_x=None), 0, None),
    ('fg_rollout_hd_policy', dict(K=0, N=2, pos_x=None), 0, None),
    ('fg_rollout_hd_policy', dict(B=-1, K=0), 0, None),
    ('fg_rollout_hd_policy', dict(B=0, K=-1), 0, None),
    ('fg_rollout_hd_policy', dict(B=-1), -1, 'B and K must be >= 0'),
    ('fg_rollout_hd_policy', dict(K=-1), -1, 'B and K must be >= 0'),
    ('fg_rollout_hd_policy', dict(B=-1, N=2), -1, 'B and K must be >= 0'),
    ('fg_rollout_hd_policy', dict(N=2), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_rollout_hd_policy', dict(N=1025), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_rollout_hd_policy', dict(pos_x=None), -1, 'fg_rollout_hd_policy: a required pointer is NULL'),
    ('fg_rollout_hd_policy', dict(reward=None), -1, 'fg_rollout_hd_policy: a required pointer is NULL'),
    ('fg_rollout_hd_policy', dict(step=None), -1, 'fg_rollout_hd_policy: a required pointer is NULL'),
    ('fg_rollout_hd_policy', dict(obs=None, reward=None), -1, 'fg_rollout_hd_policy: a required pointer is NULL'),
    ('fg_rollout_hd_policy', dict(obs=4100), -3, 'obs_seq must be 16-byte, act_seq/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_rollout_hd_policy', dict(act=4100), -3, 'obs_seq must be 16-byte, act_seq/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_rollout_hd_policy', dict(ideal_shape=4100), -3, 'obs_seq must be 16-byte, act_seq/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_rollout_hd_policy', dict(reward=None, obs=4100), -1, 'fg_rollout_hd_policy: a required pointer is NULL'),
    ('fg_rollout_hd_policy', dict(N=2, reward=None), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_rollout_hd_policy', dict(params={'obs_env_pitch': 7}), -1, 'params: obs_env_pitch must be 0 or an even number of floats >= 6 N^2'),
    ('fg_rollout_hd_policy', dict(params={'obs_env_pitch': 7}, obs=4100), -3, 'obs_seq must be 16-byte, act_seq/ideal_shape/ideal_vel 8-byte aligned'),
    ('fg_rollout_hd_policy', dict(B=0, N=10), 0, None),
    ('fg_rollout_hd_policy', dict(N=10), -2, 'fg_rollout_hd_policy: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_rollout_hd_policy', dict(N=81, per=9), -2, 'fg_rollout_hd_policy: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_rollout_hd_policy', dict(per=1), -2, 'fg_rollout_hd_policy: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_rollout_hd_policy', dict(N=2, per=2), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_rollout_hd_policy', dict(N=10, pos_x=None), -2, 'fg_rollout_hd_policy: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_rollout_hd_policy', dict(N=10, obs=4100), -2, 'fg_rollout_hd_policy: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_rollout_hd_policy', dict(B=-1, N=10), -1, 'B and K must be >= 0'),
    ('fg_rollout_hd_policy', dict(N=10, params={'obs_env_pitch': 7}), -2, 'fg_rollout_hd_policy: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_reset_hd', dict(B=0, N=1, pos_x=None), 0, None),
    ('fg_reset_hd', dict(B=-1), -1, 'B must be >= 0'),
    ('fg_reset_hd', dict(B=-1, N=1), -1, 'B must be >= 0'),
    ('fg_reset_hd', dict(N=1), -2, 'N must be in [2, 1024]'),
    ('fg_reset_hd', dict(N=5000), -2, 'N must be in [2, 1024]'),
    ('fg_reset_hd', dict(pos_x=None), -1, 'fg_reset_hd: a required pointer is NULL'),
    ('fg_reset_hd', dict(ideal_vel=None), -1, 'fg_reset_hd: a required pointer is NULL'),
    ('fg_reset_hd', dict(N=1, pos_x=None), -2, 'N must be in [2, 1024]'),
    ('fg_reset_hd_mt', dict(B=0, N=1, mt_state=None), 0, None),
    ('fg_reset_hd_mt', dict(B=-1), -1, 'B must be >= 0'),
    ('fg_reset_hd_mt', dict(B=-1, N=1), -1, 'B must be >= 0'),
    ('fg_reset_hd_mt', dict(N=1), -2, 'N must be in [2, 1024]'),
    ('fg_reset_hd_mt', dict(N=1025), -2, 'N must be in [2, 1024]'),
    ('fg_reset_hd_mt', dict(mt_state=None), -1, 'fg_reset_hd_mt: a required pointer is NULL'),
    ('fg_reset_hd_mt', dict(ideal_vel=None), -1, 'fg_reset_hd_mt: a required pointer is NULL'),
    ('fg_reset_hd_mt', dict(N=1, mt_state=None), -2, 'N must be in [2, 1024]'),
    ('fg_reset_hd_mt_done', dict(B=0, world_length=0, step=None), 0, None),
    ('fg_reset_hd_mt_done', dict(world_length=0), -1, 'fg_reset_hd_mt_done: world_length > 0 and step required'),
    ('fg_reset_hd_mt_done', dict(step=None), -1, 'fg_reset_hd_mt_done: world_length > 0 and step required'),
    ('fg_reset_hd_mt_done', dict(B=-1, world_length=0), -1, 'fg_reset_hd_mt_done: world_length > 0 and step required'),
    ('fg_reset_hd_mt_done', dict(B=-1), -1, 'B must be >= 0'),
    ('fg_reset_hd_mt_done', dict(B=-1, N=1), -1, 'B must be >= 0'),
    ('fg_reset_hd_mt_done', dict(N=1), -2, 'N must be in [2, 1024]'),
    ('fg_reset_hd_mt_done', dict(N=1025), -2, 'N must be in [2, 1024]'),
    ('fg_reset_hd_mt_done', dict(mt_state=None), -1, 'fg_reset_hd_mt: a required pointer is NULL'),
    ('fg_reset_hd_mt_done', dict(obs_env_pitch=7), -1, 'obs_env_pitch must be 0 or an even number of floats >= 6 N^2'),
    ('fg_reset_hd_mt_done', dict(obs_env_pitch=484), -1, 'obs_env_pitch must be 0 or an even number of floats >= 6 N^2'),
    ('fg_reset_hd_mt_done', dict(obs=4100), -3, 'obs must be 8-byte aligned'),
    ('fg_reset_hd_mt_done', dict(obs=4100, obs_env_pitch=7), -1, 'obs_env_pitch must be 0 or an even number of floats >= 6 N^2'),
    ('fg_reset_hd_mt_done', dict(mt_state=None, obs_env_pitch=7), -1, 'fg_reset_hd_mt: a required pointer is NULL'),
    ('fg_reset_hd_mt_done', dict(N=1, step=None), -1, 'fg_reset_hd_mt_done: world_length > 0 and step required'),
    ('fg_reset_scenario', dict(scenario=None), -1, 'scenario descriptor is NULL'),
    ('fg_reset_scenario', dict(scenario=None, B=-1, N=1), -1, 'scenario descriptor is NULL'),
    ('fg_reset_scenario', dict(scenario={'kind': 9}, N=1), -1, 'unknown scenario kind'),
    ('fg_reset_scenario', dict(scenario={'kind': 9}, B=0), -1, 'unknown scenario kind'),
    ('fg_reset_scenario', dict(scenario={'kind': 9}, B=-1), -1, 'unknown scenario kind'),
    ('fg_reset_scenario', dict(B=0, N=1, pos_x=None), 0, None),
    ('fg_reset_scenario', dict(B=-1), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_reset_scenario', dict(scenario={'num_landmarks': 0}), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_reset_scenario', dict(scenario={'num_obstacles': -1}), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_reset_scenario', dict(B=-1, N=1), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_reset_scenario', dict(N=1), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_reset_scenario', dict(N=1022), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_reset_scenario', dict(scenario={'num_landmarks': 1025}), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_reset_scenario', dict(scenario={'num_landmarks': 0}, N=1), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_reset_scenario', dict(pos_x=None), -1, 'fg_reset_scenario: a required pointer is NULL'),
    ('fg_reset_scenario', dict(landmarks=None), -1, 'fg_reset_scenario: a required pointer is NULL'),
    ('fg_reset_scenario', dict(obst_pos=None), -1, 'fg_reset_scenario: a required pointer is NULL'),
    ('fg_reset_scenario', dict(obst_vel=None), -1, 'fg_reset_scenario: a required pointer is NULL'),
    ('fg_reset_scenario', dict(landmarks=4100), -3, 'landmarks / obstacle buffers must be 8-byte aligned'),
    ('fg_reset_scenario', dict(obst_pos=4100), -3, 'landmarks / obstacle buffers must be 8-byte aligned'),
    ('fg_reset_scenario', dict(obst_vel=4100), -3, 'landmarks / obstacle buffers must be 8-byte aligned'),
    ('fg_reset_scenario', dict(pos_x=None, landmarks=4100), -1, 'fg_reset_scenario: a required pointer is NULL'),
    ('fg_reset_scenario', dict(N=1022, pos_x=None), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_reset_scenario', dict(scenario={'num_obstacles': 0}, obst_pos=None, obst_vel=4100), -3, 'landmarks / obstacle buffers must be 8-byte aligned'),
    ('fg_reset_scenario_mt', dict(scenario=None), -1, 'scenario descriptor is NULL'),
    ('fg_reset_scenario_mt', dict(scenario=None, B=-1, N=1), -1, 'scenario descriptor is NULL'),
    ('fg_reset_scenario_mt', dict(scenario={'kind': 9}, N=1), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_reset_scenario_mt', dict(scenario={'kind': 9}, B=0), 0, None),
    ('fg_reset_scenario_mt', dict(scenario={'kind': 9}, B=-1), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_reset_scenario_mt', dict(B=0, N=1, pos_x=None), 0, None),
    ('fg_reset_scenario_mt', dict(B=-1), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_reset_scenario_mt', dict(scenario={'num_landmarks': 0}), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_reset_scenario_mt', dict(scenario={'num_obstacles': -1}), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_reset_scenario_mt', dict(B=-1, N=1), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_reset_scenario_mt', dict(N=1), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_reset_scenario_mt', dict(N=1022), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_reset_scenario_mt', dict(scenario={'num_landmarks': 1025}), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_reset_scenario_mt', dict(scenario={'num_landmarks': 0}, N=1), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_reset_scenario_mt', dict(pos_x=None), -1, 'fg_reset_scenario_mt: a required pointer is NULL'),
    ('fg_reset_scenario_mt', dict(landmarks=None), -1, 'fg_reset_scenario_mt: a required pointer is NULL'),
    ('fg_reset_scenario_mt', dict(obst_pos=None), -1, 'fg_reset_scenario_mt: a required pointer is NULL'),
    ('fg_reset_scenario_mt', dict(obst_vel=None), -1, 'fg_reset_scenario_mt: a required pointer is NULL'),
    ('fg_reset_scenario_mt', dict(landmarks=4100), -3, 'landmarks / obstacle buffers must be 8-byte aligned'),
    ('fg_reset_scenario_mt', dict(obst_pos=4100), -3, 'landmarks / obstacle buffers must be 8-byte aligned'),
    ('fg_reset_scenario_mt', dict(obst_vel=4100), -3, 'landmarks / obstacle buffers must be 8-byte aligned'),
    ('fg_reset_scenario_mt', dict(pos_x=None, landmarks=4100), -1, 'fg_reset_scenario_mt: a required pointer is NULL'),
    ('fg_reset_scenario_mt', dict(N=1022, pos_x=None), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_reset_scenario_mt', dict(scenario={'num_obstacles': 0}, obst_pos=None, obst_vel=4100), -3, 'landmarks / obstacle buffers must be 8-byte aligned'),
    ('fg_reset_scenario_mt', dict(mt_state=None), -1, 'fg_reset_scenario_mt: a required pointer is NULL'),
    ('fg_reset_scenario_mt', dict(mask=None, step=None), -1, 'fg_reset_scenario_mt: the done rule needs the step counters'),
    ('fg_reset_scenario_mt', dict(mask=None, step=None, landmarks=4100), -1, 'fg_reset_scenario_mt: the done rule needs the step counters'),
    ('fg_reset_scenario_mt', dict(mask=None, step=None, pos_x=None), -1, 'fg_reset_scenario_mt: a required pointer is NULL'),
    ('fg_step_scenario', dict(scenario=None), -1, 'scenario descriptor is NULL'),
    ('fg_step_scenario', dict(params={'comm_state': 4096}), -1, 'comm_state is honoured by the formation_hd_env entry points only'),
    ('fg_step_scenario', dict(params={'comm_state': 4096}, scenario={'kind': 9}), -1, 'comm_state is honoured by the formation_hd_env entry points only'),
    ('fg_step_scenario', dict(params={'comm_state': 4096}, scenario=None), -1, 'scenario descriptor is NULL'),
    ('fg_step_scenario', dict(scenario={'kind': 9}), -1, 'unknown scenario kind'),
    ('fg_step_scenario', dict(scenario={'kind': 0}), -1, 'unknown scenario kind'),
    ('fg_step_scenario', dict(scenario={'kind': 9}, B=0), -1, 'unknown scenario kind'),
    ('fg_step_scenario', dict(scenario={'kind': 9}, B=-1), -1, 'unknown scenario kind'),
    ('fg_step_scenario', dict(B=0, N=1, pos_x=None), 0, None),
    ('fg_step_scenario', dict(B=-1), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_step_scenario', dict(scenario={'num_landmarks': 0}), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_step_scenario', dict(scenario={'num_obstacles': -1}), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_step_scenario', dict(B=-1, N=1), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_step_scenario', dict(N=1), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_step_scenario', dict(N=1022), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_step_scenario', dict(scenario={'num_landmarks': 1025}), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_step_scenario', dict(scenario={'kind': 2, 'num_obs': -1}), -1, 'bad num_obs'),
    ('fg_step_scenario', dict(scenario={'kind': 2, 'num_obs': 1025}), -1, 'bad num_obs'),
    ('fg_step_scenario', dict(scenario={'kind': 2, 'num_obs': -1}, N=1), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_step_scenario', dict(scenario={'kind': 2, 'num_obs': -1}, pos_x=None), -1, 'bad num_obs'),
    ('fg_step_scenario', dict(pos_x=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_step_scenario', dict(landmarks=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_step_scenario', dict(obs=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_step_scenario', dict(act=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_step_scenario', dict(reward=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_step_scenario', dict(obst_pos=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_step_scenario', dict(obst_vel=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_step_scenario', dict(obs=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_step_scenario', dict(landmarks=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_step_scenario', dict(act=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_step_scenario', dict(obst_pos=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_step_scenario', dict(obst_vel=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_step_scenario', dict(pos_x=None, obs=4100), -1, 'scenario step: a required pointer is NULL'),
    ('fg_step_scenario', dict(N=1022, pos_x=None), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_rollout_scenario', dict(scenario=None), -1, 'scenario descriptor is NULL'),
    ('fg_rollout_scenario', dict(params={'comm_state': 4096}), -1, 'comm_state is honoured by the formation_hd_env entry points only'),
    ('fg_rollout_scenario', dict(params={'comm_state': 4096}, scenario={'kind': 9}), -1, 'comm_state is honoured by the formation_hd_env entry points only'),
    ('fg_rollout_scenario', dict(params={'comm_state': 4096}, scenario=None), -1, 'scenario descriptor is NULL'),
    ('fg_rollout_scenario', dict(scenario={'kind': 9}), -1, 'unknown scenario kind'),
    ('fg_rollout_scenario', dict(scenario={'kind': 0}), -1, 'unknown scenario kind'),
    ('fg_rollout_scenario', dict(scenario={'kind': 9}, B=0), -1, 'unknown scenario kind'),
    ('fg_rollout_scenario', dict(scenario={'kind': 9}, B=-1), -1, 'unknown scenario kind'),
    ('fg_rollout_scenario', dict(B=0, N=1, pos_x=None), 0, None),
    ('fg_rollout_scenario', dict(B=-1), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_rollout_scenario', dict(scenario={'num_landmarks': 0}), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_rollout_scenario', dict(scenario={'num_obstacles': -1}), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_rollout_scenario', dict(B=-1, N=1), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_rollout_scenario', dict(N=1), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_rollout_scenario', dict(N=1022), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_rollout_scenario', dict(scenario={'num_landmarks': 1025}), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_rollout_scenario', dict(scenario={'kind': 2, 'num_obs': -1}), -1, 'bad num_obs'),
    ('fg_rollout_scenario', dict(scenario={'kind': 2, 'num_obs': 1025}), -1, 'bad num_obs'),
    ('fg_rollout_scenario', dict(scenario={'kind': 2, 'num_obs': -1}, N=1), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_rollout_scenario', dict(scenario={'kind': 2, 'num_obs': -1}, pos_x=None), -1, 'bad num_obs'),
    ('fg_rollout_scenario', dict(pos_x=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_rollout_scenario', dict(landmarks=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_rollout_scenario', dict(obs=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_rollout_scenario', dict(act=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_rollout_scenario', dict(reward=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_rollout_scenario', dict(obst_pos=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_rollout_scenario', dict(obst_vel=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_rollout_scenario', dict(obs=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_rollout_scenario', dict(landmarks=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_rollout_scenario', dict(act=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_rollout_scenario', dict(obst_pos=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_rollout_scenario', dict(obst_vel=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_rollout_scenario', dict(pos_x=None, obs=4100), -1, 'scenario step: a required pointer is NULL'),
    ('fg_rollout_scenario', dict(N=1022, pos_x=None), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_step_scenario', dict(do_physics=0, act=None, reward=None, obs=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_step_scenario', dict(do_physics=0, act=4100, reward=None, obs=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_rollout_scenario', dict(K=0, pos_x=None), 0, None),
    ('fg_rollout_scenario', dict(K=0, scenario=None), -1, 'scenario descriptor is NULL'),
    ('fg_rollout_scenario', dict(K=0, params=None), -1, 'params is NULL'),
    ('fg_rollout_scenario', dict(K=0, scenario={'kind': 9}, params={'comm_state': 4096}), 0, None),
    ('fg_rollout_scenario', dict(K=-2), -1, 'K >= 0 and obs_every >= 1 required'),
    ('fg_rollout_scenario', dict(K=-2, scenario={'kind': 9}), -1, 'K >= 0 and obs_every >= 1 required'),
    ('fg_rollout_scenario', dict(K=-2, params={'comm_state': 4096}), -1, 'K >= 0 and obs_every >= 1 required'),
    ('fg_rollout_scenario', dict(K=-2, B=0), -1, 'K >= 0 and obs_every >= 1 required'),
    ('fg_step_basic', dict(params={'comm_state': 4096}), -1, 'comm_state is honoured by the formation_hd_env entry points only'),
    ('fg_step_basic', dict(B=0, N=1, pos_x=None), 0, None),
    ('fg_step_basic', dict(B=-1), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_step_basic', dict(L=0), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_step_basic', dict(B=-1, N=1100), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_step_basic', dict(N=1), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_step_basic', dict(N=1100), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_step_basic', dict(L=1025), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_step_basic', dict(L=0, N=1), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_step_basic', dict(pos_x=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_step_basic', dict(obs=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_step_basic', dict(act=None), -1, 'scenario step: a required pointer is NULL'),
    ('fg_step_basic', dict(do_physics=0, act=None, reward=None, obs=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_step_basic', dict(obs=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_step_basic', dict(landmarks=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_step_basic', dict(act=4100), -3, 'obs/landmarks/act/obstacle buffers must be 8-byte aligned'),
    ('fg_step_basic', dict(landmarks=None, obs=4100), -1, 'scenario step: a required pointer is NULL'),
    ('fg_step_basic', dict(params={'comm_state': 4096}, B=-1, N=1), -1, 'comm_state is honoured by the formation_hd_env entry points only'),
    ('fg_update_comm', dict(B=0, N=0, action_c=None), 0, None),
    ('fg_update_comm', dict(B=-1), -1, 'B must be >= 0'),
    ('fg_update_comm', dict(B=-1, N=0), -1, 'B must be >= 0'),
    ('fg_update_comm', dict(N=0), -2, 'N must be in [1, 1024]'),
    ('fg_update_comm', dict(N=5000), -2, 'N must be in [1, 1024]'),
    ('fg_update_comm', dict(action_c=None), -1, 'fg_update_comm: a required pointer is NULL'),
    ('fg_update_comm', dict(comm_state=None), -1, 'fg_update_comm: a required pointer is NULL'),
    ('fg_update_comm', dict(action_c=4100), -3, 'action_c and comm_state must be 8-byte aligned'),
    ('fg_update_comm', dict(comm_state=4100), -3, 'action_c and comm_state must be 8-byte aligned'),
    ('fg_update_comm', dict(action_c=None, comm_state=4100), -1, 'fg_update_comm: a required pointer is NULL'),
    ('fg_update_comm', dict(N=0, action_c=None), -2, 'N must be in [1, 1024]'),
    ('fg_update_comm_dim', dict(dim_c=2, B=-1), -1, 'B must be >= 0'),
    ('fg_update_comm_dim', dict(dim_c=2, N=0), -2, 'N must be in [1, 1024]'),
    ('fg_update_comm_dim', dict(dim_c=2, action_c=None), -1, 'fg_update_comm: a required pointer is NULL'),
    ('fg_update_comm_dim', dict(dim_c=2, action_c=4100), -3, 'action_c and comm_state must be 8-byte aligned'),
    ('fg_update_comm_dim', dict(dim_c=2, params=None), -1, 'params is NULL'),
    ('fg_update_comm_dim', dict(B=0, N=0, action_c=None), 0, None),
    ('fg_update_comm_dim', dict(dim_c=0, N=0, action_c=None), 0, None),
    ('fg_update_comm_dim', dict(B=-1), -1, 'B >= 0 and 0 <= dim_c <= 4096 required'),
    ('fg_update_comm_dim', dict(dim_c=-1), -1, 'B >= 0 and 0 <= dim_c <= 4096 required'),
    ('fg_update_comm_dim', dict(dim_c=4097), -1, 'B >= 0 and 0 <= dim_c <= 4096 required'),
    ('fg_update_comm_dim', dict(B=-1, N=0), -1, 'B >= 0 and 0 <= dim_c <= 4096 required'),
    ('fg_update_comm_dim', dict(B=0, dim_c=-1), 0, None),
    ('fg_update_comm_dim', dict(N=0), -2, 'N must be in [1, 1024]'),
    ('fg_update_comm_dim', dict(N=5000), -2, 'N must be in [1, 1024]'),
    ('fg_update_comm_dim', dict(action_c=None), -1, 'fg_update_comm_dim: a required pointer is NULL'),
    ('fg_update_comm_dim', dict(comm_state=None), -1, 'fg_update_comm_dim: a required pointer is NULL'),
    ('fg_update_comm_dim', dict(action_c=4098), -3, 'action_c and comm_state must be 4-byte aligned'),
    ('fg_update_comm_dim', dict(comm_state=4097), -3, 'action_c and comm_state must be 4-byte aligned'),
    ('fg_update_comm_dim', dict(action_c=None, comm_state=4098), -1, 'fg_update_comm_dim: a required pointer is NULL'),
    ('fg_update_comm_dim', dict(N=0, action_c=None), -2, 'N must be in [1, 1024]'),
    ('fg_update_comm_dim', dict(dim_c=-1, N=0), -1, 'B >= 0 and 0 <= dim_c <= 4096 required'),
    ('fg_policy_bfs', dict(B=0, N=2, act=None), 0, None),
    ('fg_policy_bfs', dict(B=-1), -1, 'B must be >= 0'),
    ('fg_policy_bfs', dict(B=-1, N=2), -1, 'B must be >= 0'),
    ('fg_policy_bfs', dict(N=2), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_policy_bfs', dict(N=2, per=2), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_policy_bfs', dict(N=1025), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_policy_bfs', dict(N=10), -2, 'fg_policy_bfs: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_policy_bfs', dict(N=81, per=9), -2, 'fg_policy_bfs: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_policy_bfs', dict(per=1), -2, 'fg_policy_bfs: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_policy_bfs', dict(N=10, act=None), -2, 'fg_policy_bfs: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_policy_bfs', dict(act=None), -1, 'fg_policy_bfs: a required pointer is NULL'),
    ('fg_policy_bfs', dict(act=4100), -3, 'obs and act must be 8-byte aligned'),
    ('fg_policy_bfs', dict(N=10, act=4100), -2, 'fg_policy_bfs: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_policy_bfs_state', dict(B=0, N=2, act=None), 0, None),
    ('fg_policy_bfs_state', dict(B=-1), -1, 'B must be >= 0'),
    ('fg_policy_bfs_state', dict(B=-1, N=2), -1, 'B must be >= 0'),
    ('fg_policy_bfs_state', dict(N=2), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_policy_bfs_state', dict(N=2, per=2), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_policy_bfs_state', dict(N=1025), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_policy_bfs_state', dict(N=10), -2, 'fg_policy_bfs_state: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_policy_bfs_state', dict(N=81, per=9), -2, 'fg_policy_bfs_state: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_policy_bfs_state', dict(per=1), -2, 'fg_policy_bfs_state: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_policy_bfs_state', dict(N=10, act=None), -2, 'fg_policy_bfs_state: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_policy_bfs_state', dict(act=None), -1, 'fg_policy_bfs_state: a required pointer is NULL'),
    ('fg_policy_bfs_state', dict(act=4100), -3, 'ideal_shape, ideal_vel and act must be 8-byte aligned'),
    ('fg_policy_bfs_state', dict(N=10, act=4100), -2, 'fg_policy_bfs_state: N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_policy_bfs', dict(obs=None), -1, 'fg_policy_bfs: a required pointer is NULL'),
    ('fg_policy_bfs', dict(obs=None, act=4100), -1, 'fg_policy_bfs: a required pointer is NULL'),
    ('fg_policy_bfs', dict(obs_env_stride=7), -1, 'fg_policy_bfs: obs_env_stride must be even and >= 6 N'),
    ('fg_policy_bfs', dict(obs_env_stride=52), -1, 'fg_policy_bfs: obs_env_stride must be even and >= 6 N'),
    ('fg_policy_bfs', dict(obs_env_stride=7, obs=4100), -1, 'fg_policy_bfs: obs_env_stride must be even and >= 6 N'),
    ('fg_policy_bfs', dict(obs=4100), -3, 'obs and act must be 8-byte aligned'),
    ('fg_policy_bfs', dict(obs=None, obs_env_stride=7), -1, 'fg_policy_bfs: a required pointer is NULL'),
    ('fg_policy_bfs_state', dict(pos_x=None), -1, 'fg_policy_bfs_state: a required pointer is NULL'),
    ('fg_policy_bfs_state', dict(ideal_vel=None), -1, 'fg_policy_bfs_state: a required pointer is NULL'),
    ('fg_policy_bfs_state', dict(ideal_shape=4100), -3, 'ideal_shape, ideal_vel and act must be 8-byte aligned'),
    ('fg_policy_bfs_state', dict(ideal_vel=4100), -3, 'ideal_shape, ideal_vel and act must be 8-byte aligned'),
    ('fg_policy_bfs_state', dict(pos_x=None, act=4100), -1, 'fg_policy_bfs_state: a required pointer is NULL'),
    ('fg_decode_actions', dict(mode=0), -1, 'fg_decode_actions: unknown mode'),
    ('fg_decode_actions', dict(mode=4), -1, 'fg_decode_actions: unknown mode'),
    ('fg_decode_actions', dict(mode=0, count=0), -1, 'fg_decode_actions: unknown mode'),
    ('fg_decode_actions', dict(mode=0, count=-3), -1, 'fg_decode_actions: unknown mode'),
    ('fg_decode_actions', dict(count=0, action=None, u_out=4100), 0, None),
    ('fg_decode_actions', dict(count=-3), -1, 'fg_decode_actions: count out of range'),
    ('fg_decode_actions', dict(count=274877906945), -1, 'fg_decode_actions: count out of range'),
    ('fg_decode_actions', dict(count=-3, action=None), -1, 'fg_decode_actions: count out of range'),
    ('fg_decode_actions', dict(action=None), -1, 'fg_decode_actions: a required pointer is NULL'),
    ('fg_decode_actions', dict(u_out=None), -1, 'fg_decode_actions: a required pointer is NULL'),
    ('fg_decode_actions', dict(u_out=4100), -3, 'fg_decode_actions: buffers must be 8-byte aligned'),
    ('fg_decode_actions', dict(action=4100), -3, 'fg_decode_actions: buffers must be 8-byte aligned'),
    ('fg_decode_actions', dict(action=4100, mode=2, u_out=4100), -3, 'fg_decode_actions: buffers must be 8-byte aligned'),
    ('fg_decode_actions', dict(action=None, u_out=4100), -1, 'fg_decode_actions: a required pointer is NULL'),
    ('fg_actor_noise', dict(B=-1), -1, 'fg_actor_noise: B >= 0 and 1 <= N < 2^29 required'),
    ('fg_actor_noise', dict(N=0), -1, 'fg_actor_noise: B >= 0 and 1 <= N < 2^29 required'),
    ('fg_actor_noise', dict(N=536870912), -1, 'fg_actor_noise: B >= 0 and 1 <= N < 2^29 required'),
    ('fg_actor_noise', dict(B=-1, eps=None), -1, 'fg_actor_noise: B >= 0 and 1 <= N < 2^29 required'),
    ('fg_actor_noise', dict(eps=None), -1, 'fg_actor_noise: eps is NULL'),
    ('fg_actor_noise', dict(eps=4100), -3, 'fg_actor_noise: eps must be 8-byte aligned'),
    ('fg_actor_noise', dict(B=0, eps=None), -1, 'fg_actor_noise: eps is NULL'),
    ('fg_actor_noise', dict(B=0, eps=4100), -3, 'fg_actor_noise: eps must be 8-byte aligned'),
    ('fg_actor_noise', dict(B=0), 0, None),
    ('fg_actor_noise', dict(params=None, B=-1, eps=None), -1, 'params is NULL'),
    ('fg_kernel_config', dict(N=1), -2, 'N must be in [2, 1024]'),
    ('fg_kernel_config', dict(N=1025), -2, 'N must be in [2, 1024]'),
    ('fg_describe_launch', dict(out=None), -1, 'fg_describe_launch: out buffer required'),
    ('fg_describe_launch', dict(out=None, params=None), -1, 'fg_describe_launch: out buffer required'),
    ('fg_describe_launch', dict(params=None, B=0), -1, 'params is NULL'),
    ('fg_describe_launch', dict(B=0), -1, 'fg_describe_launch: B > 0 and K >= 0 required'),
    ('fg_describe_launch', dict(K=-1), -1, 'fg_describe_launch: B > 0 and K >= 0 required'),
    ('fg_describe_launch', dict(B=0, N=2), -1, 'fg_describe_launch: B > 0 and K >= 0 required'),
    ('fg_describe_launch', dict(N=2), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_describe_launch', dict(N=1025), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_describe_launch', dict(N=2, per=3), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_describe_launch', dict(N=2, params={'obs_env_pitch': 7}), -2, 'formation_hd_env needs 3 <= N <= 1024'),
    ('fg_describe_launch', dict(params={'obs_env_pitch': 7}), -1, 'params: obs_env_pitch must be 0 or an even number of floats >= 6 N^2'),
    ('fg_describe_launch', dict(params={'obs_env_pitch': 7}, N=10, per=3), -1, 'params: obs_env_pitch must be 0 or an even number of floats >= 6 N^2'),
    ('fg_describe_launch', dict(N=10, per=3), -2, 'N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_describe_launch', dict(N=81, per=9), -2, 'N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_describe_launch', dict(per=1), -2, 'N must be per_layer^L with 2 <= per_layer <= 8'),
    ('fg_describe_launch', dict(B=0, scenario={}), -1, 'fg_describe_launch: B > 0 and K >= 0 required'),
    ('fg_describe_launch', dict(scenario={'kind': 9}), -1, 'unknown scenario kind'),
    ('fg_describe_launch', dict(scenario={'kind': 9}, params={'comm_state': 4096}), -1, 'comm_state is honoured by the formation_hd_env entry points only'),
    ('fg_describe_launch', dict(params={'comm_state': 4096}, scenario={}), -1, 'comm_state is honoured by the formation_hd_env entry points only'),
    ('fg_describe_launch', dict(scenario={'num_landmarks': 0}), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_describe_launch', dict(scenario={'num_obstacles': -1}), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_describe_launch', dict(N=1, scenario={}), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_describe_launch', dict(N=1022, scenario={}), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_describe_launch', dict(scenario={'num_landmarks': 1025}), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_describe_launch', dict(scenario={'num_landmarks': 0}, N=1), -1, 'B >= 0, L > 0, M >= 0 required'),
    ('fg_describe_launch', dict(scenario={'kind': 2, 'num_obs': -1}), -1, 'bad num_obs'),
    ('fg_describe_launch', dict(scenario={'kind': 2, 'num_obs': 1025}, N=1022), -2, 'scenario kernel needs 2 <= N, N + M <= 1024, L <= 1024'),
    ('fg_describe_scenario_actor_launch', dict(out=None), -1, 'fg_describe_scenario_actor_launch: out buffer required'),
    ('fg_describe_scenario_actor_launch', dict(out=None, params=None), -1, 'fg_describe_scenario_actor_launch: out buffer required'),
    ('fg_rollout_scenario_actor', dict(scenario=None), -1, 'fg_rollout_scenario_actor: scenario descriptor is NULL'),
    ('fg_rollout_scenario_actor', dict(scenario=None, actor=None, B=-1), -1, 'fg_rollout_scenario_actor: scenario descriptor is NULL'),
    ('fg_rollout_scenario_actor', dict(B=-1), -1, 'fg_rollout_scenario_actor: B >= 0 and K >= 1 required'),
    ('fg_rollout_scenario_actor', dict(K=0), -1, 'fg_rollout_scenario_actor: B >= 0 and K >= 1 required'),
    ('fg_rollout_scenario_actor', dict(B=-1, scenario={'kind': 9}), -1, 'fg_rollout_scenario_actor: B >= 0 and K >= 1 required'),
    ('fg_rollout_scenario_actor', dict(scenario={'kind': 9}), -1, 'fg_rollout_scenario_actor: unknown scenario kind'),
    ('fg_rollout_scenario_actor', dict(scenario={'kind': 9}, actor=None), -1, 'fg_rollout_scenario_actor: unknown scenario kind'),
    ('fg_rollout_scenario_actor', dict(actor=None), -1, 'fg_rollout_scenario_actor: actor is NULL'),
    ('fg_rollout_scenario_actor', dict(actor={'hidden': 128}), -1, 'fg_rollout_scenario_actor: hidden must be 32 or 64'),
    ('fg_rollout_scenario_actor', dict(actor={'hidden': 48}), -1, 'fg_rollout_scenario_actor: hidden must be 32 or 64'),
    ('fg_rollout_scenario_actor', dict(actor={'w2': None}), -1, 'fg_rollout_scenario_actor: a weight pointer is NULL'),
    ('fg_rollout_scenario_actor', dict(actor={'b3': 4098}), -3, 'fg_rollout_scenario_actor: weights, log_std and logp must be 4-byte aligned'),
    ('fg_rollout_scenario_actor', dict(log_std=4098), -3, 'fg_rollout_scenario_actor: weights, log_std and logp must be 4-byte aligned'),
    ('fg_rollout_scenario_actor', dict(actor={'w2': None, 'b3': 4098}), -1, 'fg_rollout_scenario_actor: a weight pointer is NULL'),
    ('fg_rollout_scenario_actor', dict(actor={'hidden': 48}, params={'comm_state': 4096}), -1, 'fg_rollout_scenario_actor: hidden must be 32 or 64'),
    ('fg_rollout_scenario_actor', dict(params={'agent_props': 4096}), -1, 'fg_rollout_scenario_actor: per-agent properties, communication and variant 1 are not supported'),
    ('fg_rollout_scenario_actor', dict(params={'comm_state': 4096}), -1, 'fg_rollout_scenario_actor: per-agent properties, communication and variant 1 are not supported'),
    ('fg_rollout_scenario_actor', dict(scenario={'variant': 1}), -1, 'fg_rollout_scenario_actor: per-agent properties, communication and variant 1 are not supported'),
    ('fg_rollout_scenario_actor', dict(N=5), -2, 'fg_rollout_scenario_actor: (scenario, N, landmarks, obstacles, num_obs) is not one of the reference shapes'),
    ('fg_rollout_scenario_actor', dict(scenario={'num_landmarks': 5}), -2, 'fg_rollout_scenario_actor: (scenario, N, landmarks, obstacles, num_obs) is not one of the reference shapes'),
    ('fg_rollout_scenario_actor', dict(N=5, scenario={'variant': 1}), -1, 'fg_rollout_scenario_actor: per-agent properties, communication and variant 1 are not supported'),
    ('fg_describe_scenario_actor_launch', dict(scenario=None), -1, 'fg_rollout_scenario_actor: scenario descriptor is NULL'),
    ('fg_describe_scenario_actor_launch', dict(scenario=None, actor=None, B=-1), -1, 'fg_rollout_scenario_actor: scenario descriptor is NULL'),
    ('fg_describe_scenario_actor_launch', dict(B=-1), -1, 'fg_rollout_scenario_actor: B >= 0 and K >= 1 required'),
    ('fg_describe_scenario_actor_launch', dict(K=0), -1, 'fg_rollout_scenario_actor: B >= 0 and K >= 1 required'),
    ('fg_describe_scenario_actor_launch', dict(B=-1, scenario={'kind': 9}), -1, 'fg_rollout_scenario_actor: B >= 0 and K >= 1 required'),
    ('fg_describe_scenario_actor_launch', dict(scenario={'kind': 9}), -1, 'fg_rollout_scenario_actor: unknown scenario kind'),
    ('fg_describe_scenario_actor_launch', dict(scenario={'kind': 9}, actor=None), -1, 'fg_rollout_scenario_actor: unknown scenario kind'),
    ('fg_describe_scenario_actor_launch', dict(actor=None), -1, 'fg_rollout_scenario_actor: actor is NULL'),
    ('fg_describe_scenario_actor_launch', dict(actor={'hidden': 128}), -1, 'fg_rollout_scenario_actor: hidden must be 32 or 64'),
    ('fg_describe_scenario_actor_launch', dict(actor={'hidden': 48}), -1, 'fg_rollout_scenario_actor: hidden must be 32 or 64'),
    ('fg_describe_scenario_actor_launch', dict(actor={'w2': None}), -1, 'fg_rollout_scenario_actor: a weight pointer is NULL'),
    ('fg_describe_scenario_actor_launch', dict(actor={'b3': 4098}), -3, 'fg_rollout_scenario_actor: weights, log_std and logp must be 4-byte aligned'),
    ('fg_describe_scenario_actor_launch', dict(log_std=4098), -3, 'fg_rollout_scenario_actor: weights, log_std and logp must be 4-byte aligned'),
    ('fg_describe_scenario_actor_launch', dict(actor={'w2': None, 'b3': 4098}), -1, 'fg_rollout_scenario_actor: a weight pointer is NULL'),
    ('fg_describe_scenario_actor_launch', dict(actor={'hidden': 48}, params={'comm_state': 4096}), -1, 'fg_rollout_scenario_actor: hidden must be 32 or 64'),
    ('fg_describe_scenario_actor_launch', dict(params={'agent_props': 4096}), -1, 'fg_rollout_scenario_actor: per-agent properties, communication and variant 1 are not supported'),
    ('fg_describe_scenario_actor_launch', dict(params={'comm_state': 4096}), -1, 'fg_rollout_scenario_actor: per-agent properties, communication and variant 1 are not supported'),
    ('fg_describe_scenario_actor_launch', dict(scenario={'variant': 1}), -1, 'fg_rollout_scenario_actor: per-agent properties, communication and variant 1 are not supported'),
    ('fg_describe_scenario_actor_launch', dict(N=5), -2, 'fg_rollout_scenario_actor: (scenario, N, landmarks, obstacles, num_obs) is not one of the reference shapes'),
    ('fg_describe_scenario_actor_launch', dict(scenario={'num_landmarks': 5}), -2, 'fg_rollout_scenario_actor: (scenario, N, landmarks, obstacles, num_obs) is not one of the reference shapes'),
    ('fg_describe_scenario_actor_launch', dict(N=5, scenario={'variant': 1}), -1, 'fg_rollout_scenario_actor: per-agent properties, communication and variant 1 are not supported'),
    ('fg_rollout_scenario_actor', dict(logp=4098), -3, 'fg_rollout_scenario_actor: weights, log_std and logp must be 4-byte aligned'),
    ('fg_rollout_scenario_actor', dict(log_std=None), -1, 'fg_rollout_scenario_actor: logp without log_std'),
    ('fg_rollout_scenario_actor', dict(log_std=None, actor={'hidden': 48}), -1, 'fg_rollout_scenario_actor: hidden must be 32 or 64'),
    ('fg_rollout_scenario_actor', dict(log_std=None, pos_x=None), -1, 'fg_rollout_scenario_actor: logp without log_std'),
    ('fg_rollout_scenario_actor', dict(pos_x=None), -1, 'fg_rollout_scenario_actor: a required pointer is NULL'),
    ('fg_rollout_scenario_actor', dict(step=None), -1, 'fg_rollout_scenario_actor: a required pointer is NULL'),
    ('fg_rollout_scenario_actor', dict(reward=None), -1, 'fg_rollout_scenario_actor: a required pointer is NULL'),
    ('fg_rollout_scenario_actor', dict(act_out=None), -1, 'fg_rollout_scenario_actor: a required pointer is NULL'),
    ('fg_rollout_scenario_actor', dict(obst_pos=None), -1, 'fg_rollout_scenario_actor: a required pointer is NULL'),
    ('fg_rollout_scenario_actor', dict(obs=4100), -3, 'fg_rollout_scenario_actor: obs/landmarks/act_out/obstacle buffers must be 8-byte aligned'),
    ('fg_rollout_scenario_actor', dict(act_out=4100), -3, 'fg_rollout_scenario_actor: obs/landmarks/act_out/obstacle buffers must be 8-byte aligned'),
    ('fg_rollout_scenario_actor', dict(obst_vel=4100), -3, 'fg_rollout_scenario_actor: obs/landmarks/act_out/obstacle buffers must be 8-byte aligned'),
    ('fg_rollout_scenario_actor', dict(pos_x=None, obs=4100), -1, 'fg_rollout_scenario_actor: a required pointer is NULL'),
    ('fg_rollout_scenario_actor', dict(N=5, pos_x=None), -1, 'fg_rollout_scenario_actor: a required pointer is NULL'),
    ('fg_rollout_scenario_actor', dict(N=5, obs=4100), -3, 'fg_rollout_scenario_actor: obs/landmarks/act_out/obstacle buffers must be 8-byte aligned'),
    ('fg_rollout_scenario_actor', dict(B=0), 0, None),
    ('fg_rollout_scenario_actor', dict(B=0, N=5), -2, 'fg_rollout_scenario_actor: (scenario, N, landmarks, obstacles, num_obs) is not one of the reference shapes'),
    ('fg_rollout_scenario_actor', dict(B=0, pos_x=None), -1, 'fg_rollout_scenario_actor: a required pointer is NULL'),
    ('fg_rollout_scenario_actor', dict(B=0, obs=4100), -3, 'fg_rollout_scenario_actor: obs/landmarks/act_out/obstacle buffers must be 8-byte aligned'),
    ('fg_rollout_scenario_actor', dict(scenario={'num_obstacles': 0}, obst_pos=None, obst_vel=None, N=5), -2, 'fg_rollout_scenario_actor: (scenario, N, landmarks, obstacles, num_obs) is not one of the reference shapes'),
    ('fg_describe_scenario_actor_launch', dict(B=0), -1, 'fg_describe_scenario_actor_launch: B > 0 required'),
    ('fg_describe_scenario_actor_launch', dict(B=0, N=5), -1, 'fg_describe_scenario_actor_launch: B > 0 required'),
    ('fg_describe_scenario_actor_launch', dict(B=0, actor=None), -1, 'fg_rollout_scenario_actor: actor is NULL'),
]


def test_entries_fail_in_their_own_order_with_their_own_text(lib):
    seen = set()
    for entry, wrong, status, text in CABI_BAD_CALLS:
        assert (status == 0) == (text is None), (entry, wrong)
        rc, got = _cabi_call(lib, entry, **wrong)
        assert rc == status and (text is None or got == text), (entry, wrong, rc, got)
        seen.add(entry)
    assert seen == set(CABI_ENTRIES)


def test_no_cpu_fallback(monkeypatch):
    import formation_gym
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            formation_gym.make_env("formation_hd_env", False, 3, device="cpu")
    with pytest.raises(FileNotFoundError):
        formation_gym.make_env("no_such_scenario", False, 3)
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "LIB_PATH", "/nonexistent/libformation_hip.so")
    with pytest.raises(_native.FormationHipError, match="no CPU fallback"):
        _native.load()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "gym-formation_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".hpp", ".sh")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src, "%s mentions the oracle" % f


def test_bench_cli_and_cpp_example_build(tmp_path):
    """bench.py parses its contract flags without touching a GPU, and the plain C++ consumer of the C ABI
    (examples/c_abi_rollout.cpp) compiles and links against the header and the built library."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--mode", "--chunk"):
        assert flag in out.stdout
    lib = os.path.join(root, "gym-formation_amd", "lib")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "c_abi_rollout")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-I", os.path.join(root, "include"),
                    os.path.join(root, "examples", "c_abi_rollout.cpp"), "-L", lib, "-lformation_hip",
                    "-Wl,-rpath," + lib, "-o", exe], check=True, capture_output=True, timeout=600)
    assert os.path.getsize(exe) > 0


def test_bench_lists_its_full_option():
    """Everything beside the headline sits behind `bench.py --full` (a plain run is the headline alone)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0
    assert "--full" in out.stdout and "--quick" in out.stdout


def test_observation_pitch_detection_is_host_logic():
    """Scenario.obs_env_pitch: which observation tensors the kernels can be told about (contiguous -> 0, a uniform even
    env pitch >= 6 N^2 -> that pitch, anything else refused).  Pure stride arithmetic: runs on CPU tensors."""
    import importlib.util
    import torch
    spec = importlib.util.spec_from_file_location(
        "fg_hd_scn", os.path.join(ROOT, "gym-formation_amd", "formation_gym", "envs", "formation_hd_env.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    pitch_of = mod.Scenario.obs_env_pitch
    N, B, K = 9, 5, 3
    D = 6 * N
    assert pitch_of(None, N) == 0
    assert pitch_of(torch.zeros((B, N, D)), N) == 0 and pitch_of(torch.zeros((K, B, N, D)), N) == 0
    padded = torch.zeros((B, N * D + 26))[:, :N * D].view(B, N, D)
    assert pitch_of(padded, N) == N * D + 26
    padded4 = torch.zeros((K, B, N * D + 32))[:, :, :N * D].view(K, B, N, D)
    assert pitch_of(padded4, N) == N * D + 32
    assert pitch_of(padded4[:2], N) == N * D + 32                           # a leading slice keeps the slot stride
    assert pitch_of(torch.zeros((2 * B, N, D))[::2], N) == 2 * N * D        # every other env: a uniform pitch of 2 blocks
    one = torch.zeros((K, 1, N * D + 32))[:, :, :N * D].view(K, 1, N, D)    # B = 1: the size-1 env axis has no stride of
    assert pitch_of(one, N) == N * D + 32                                   # its own, the slot stride IS the pitch
    assert pitch_of(torch.zeros((1, N * D + 32))[:, :N * D].view(1, N, D), N) == 0 and pitch_of(one[:1], N) == 0
    for bad in (torch.zeros((B, N * D + 1))[:, :N * D].view(B, N, D),     # odd pitch
                torch.zeros((B, N, D + 2))[:, :, :D],                     # padded ROWS
                torch.zeros((2 * K, B, N * D + 32))[::2, :, :N * D].view(K, B, N, D)):   # step slots not B pitches apart
        with pytest.raises(ValueError):
            pitch_of(bad, N)
