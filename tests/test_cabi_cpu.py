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
