"""CPU checks of the 16-bit observation launches (`fg_rollout_hd_obs16`, `fg_rollout_hd_policy_obs16`): the symbols, the dry
run's twelve instantiations and their resources, argument checks that touch no device, the fp32 dispatch left alone, and which
route `env.obs_path` answers on a stand-in env."""
import ctypes
import re
import types

import pytest
import torch

from formation_gym import _native, load_scenario
from formation_gym.environment import MultiAgentEnv

from . import isa_scan

OBS16 = ("fg_rollout_hd_obs16", "fg_rollout_hd_policy_obs16", "fg_describe_obs16_launch")
WR = {_native.FG_OBS_F16: 65, _native.FG_OBS_BF16: 66}                 # FG_WR_OBS_F16 / FG_WR_OBS_BF16 (fg_obs_writers.hpp)
# (N, G, TP, TW, E): the fp32 default geometry of each class
GEOMETRY = {27: (32, 512, 256, 16), 9: (16, 64, 128, 4), 3: (4, 64, 128, 16)}
COMBOS = [(N, per, fmt) for N in (3, 9, 27) for per in (0, 3) for fmt in (_native.FG_OBS_F16, _native.FG_OBS_BF16)]


@pytest.fixture(scope="module")
def lib():
    _native.build()
    return _native.load()


def _params(**kw):
    base = dict(dt=0.1, damping=0.25, contact_force=100.0, contact_margin=1e-3, sensitivity=5.0, mass=1.0, dist_min=0.03,
                collide_thresh=0.015, world_length=100, auto_reset=1)
    base.update(kw)
    return _native.FgParams(**base)


def _describe(lib, params, fmt, B, N, K, per=0, obs_every=1):
    buf = ctypes.create_string_buffer(512)
    rc = lib.fg_describe_obs16_launch(params, fmt, B, N, K, per, obs_every, buf, len(buf))
    return rc, buf.value.decode().strip()


def test_symbols_and_abi(lib):
    for name in OBS16:
        assert name in _native.SIGNATURES
        assert hasattr(lib, name)
    assert lib.fg_abi_version() == _native.ABI_VERSION == 8


def test_describe_names_twelve_instantiations_that_are_in_the_library(lib):
    names = set()
    for N, per, fmt in COMBOS:
        B = 1000
        rc, text = _describe(lib, _params(), fmt, B, N, 20, per)
        assert rc == 0, (N, per, fmt, lib.fg_last_error())
        m = re.fullmatch(r"rollout_kernel<([\d,]+)> grid (\d+) lds (\d+);", text)
        assert m, text
        targs = [int(x) for x in m.group(1).split(",")]
        G, TP, TW, E = GEOMETRY[N]
        assert targs == [N, G, TP, TW, E, WR[fmt], per, 0], text
        assert int(m.group(2)) == -(-B // E)
        assert 0 < int(m.group(3)) <= 160 * 1024
        names.add("fg::rollout_kernel<%s, false>" % ", ".join(str(x) for x in targs[:-1]))
    assert len(names) == 12
    built = [k for k in isa_scan.kernel_resources(_native.LIB_PATH)]
    for n in names:
        hit = [k for k in built if n in k["demangled"]]
        assert len(hit) == 1, n
        k = hit[0]
        assert k["private_segment"] == 0 and k["vgpr_spill"] == 0, (n, k)
        assert k["vgpr"] <= 168, (n, k["vgpr"])


def test_argument_checks_touch_no_device(lib):
    P = _params()
    p = 4096                                               # never dereferenced: every call below fails (or has nothing to do) first
    ptrs = [p] * 12

    def roll(params=P, fmt=_native.FG_OBS_F16, B=8, N=9, K=4, ptrs=ptrs):
        return lib.fg_rollout_hd_obs16(params, fmt, B, N, K, *ptrs, 1, None)

    def pol(params=P, fmt=_native.FG_OBS_BF16, B=8, N=9, K=4, per=3, ptrs=ptrs):
        return lib.fg_rollout_hd_policy_obs16(params, fmt, B, N, K, per, *ptrs, 1, None)

    for call in (roll, pol):
        for N in (4, 81):
            assert call(N=N) == _native.FG_ERR_UNSUPPORTED_N
            assert b"3, 9 or 27" in lib.fg_last_error()
        for fmt in (0, 3):
            assert call(fmt=fmt) == _native.FG_ERR_BAD_ARG
            assert b"obs_format" in lib.fg_last_error()
        assert call(K=1) == _native.FG_ERR_BAD_ARG
        assert call(params=_params(obs_env_pitch=512)) == _native.FG_ERR_BAD_ARG
        assert b"pitch" in lib.fg_last_error()
        assert call(params=_params(agent_props=4096)) == _native.FG_ERR_BAD_ARG
        for opt in (dict(u_noise=0.1), dict(max_speed=0.5), dict(accel=1.0), dict(num_walls=1), dict(comm_state=4096)):
            assert call(params=_params(**opt)) == _native.FG_ERR_BAD_ARG, opt
        mis = list(ptrs); mis[8] = 4100                    # obs_seq
        assert call(ptrs=mis) == _native.FG_ERR_ALIGNMENT
        assert b"aligned" in lib.fg_last_error()
        assert call(B=0, ptrs=[None] * 12) == _native.FG_OK
    assert pol(per=2) == _native.FG_ERR_UNSUPPORTED_N
    # the dry run: the same codes
    assert _describe(lib, P, _native.FG_OBS_F16, 8, 4, 4)[0] == _native.FG_ERR_UNSUPPORTED_N
    assert _describe(lib, P, _native.FG_OBS_F16, 8, 81, 4)[0] == _native.FG_ERR_UNSUPPORTED_N
    assert _describe(lib, P, 0, 8, 9, 4)[0] == _native.FG_ERR_BAD_ARG
    assert _describe(lib, P, 3, 8, 9, 4)[0] == _native.FG_ERR_BAD_ARG
    assert _describe(lib, P, _native.FG_OBS_F16, 8, 9, 1)[0] == _native.FG_ERR_BAD_ARG
    assert _describe(lib, _params(obs_env_pitch=512), _native.FG_OBS_F16, 8, 9, 4)[0] == _native.FG_ERR_BAD_ARG
    assert _describe(lib, _params(agent_props=4096), _native.FG_OBS_F16, 8, 9, 4)[0] == _native.FG_ERR_BAD_ARG
    assert _describe(lib, P, _native.FG_OBS_F16, 8, 9, 4, per=2)[0] == _native.FG_ERR_UNSUPPORTED_N


def test_the_fp32_dispatch_answers_as_before(lib):
    """The fp32 launches of the same agent counts still go where tests/golden/dispatch.json says (the whole grid:
    tests/test_dispatch_snapshot.py); none of them names a 16-bit writer."""
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispatch.json")) as fh:
        want = json.load(fh)
    for N in (3, 9, 27):
        for B in (64, 4096, 65536):
            for K in (2, 20, 128):
                for per in (0, 3):
                    buf = ctypes.create_string_buffer(2048)
                    assert lib.fg_describe_launch(_params(), None, B, N, K, per, 1, 0, buf, len(buf)) == 0
                    got = buf.value.decode().strip()
                    key = "hd N=%d B=%d K=%d placed=0" % (N, B, K) + (" per=3" if per else "")
                    assert got == want[key], key
                    assert not re.search(r"rollout_kernel<(\d+,){5}(65|66),", got)


# ---- env.obs_path on a stand-in env: the scenario object, a world that answers what `Scenario.params` asks, no device ----
def _standin(name, N, **options):
    sc = load_scenario(name)
    sc._seed = 1
    world = types.SimpleNamespace(
        agents=[types.SimpleNamespace(size=0.03) for _ in range(N)], num_envs=64, dim_c=2,
        any_non_silent=lambda: False,
        native_params=lambda **kw: _params(**dict(options, collide_thresh=kw.get("collide_thresh", 0.015))))
    return types.SimpleNamespace(scenario=sc, world=world, post_step_callback=None)


def _obs_path(env, dtype, policy=False):
    return MultiAgentEnv.obs_path(env, dtype, policy)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_obs_path(lib, dtype):
    for N in (3, 9, 27):
        for policy in (False, True):
            assert _obs_path(_standin("formation_hd_env", N), dtype, policy) == "fused", (N, policy)
    assert _obs_path(_standin("formation_hd_env", 4), dtype) == "cast"
    assert _obs_path(_standin("formation_hd_env", 81), dtype, True) == "cast"
    for opt in (dict(u_noise=0.1), dict(max_speed=0.5), dict(num_walls=1), dict(agent_props=4096)):
        assert _obs_path(_standin("formation_hd_env", 9, **opt), dtype) == "cast", opt
    assert _obs_path(_standin("basic_formation_env", 3), dtype) == "cast"              # a landmark scenario
    cb = _standin("formation_hd_env", 9)
    cb.post_step_callback = lambda world: None                                         # a host function after every step
    assert _obs_path(cb, dtype) == "cast"


def test_obs_dtype_must_be_a_16_bit_float():
    env = _standin("formation_hd_env", 9)
    for bad in (torch.float64, torch.float32, torch.int16, None):
        with pytest.raises(ValueError):
            _obs_path(env, bad)
    with pytest.raises(ValueError):
        _native.obs_format(torch.float64)
    assert _native.obs_format(None) == 0
    assert (_native.obs_format(torch.float16), _native.obs_format(torch.bfloat16)) == (_native.FG_OBS_F16, _native.FG_OBS_BF16)
