"""CPU checks of the recurrent rollout that keeps its per-step hidden states (`fg_rollout_hd_actor_gru_states`,
`rollout_actor(..., rnn_states_every=S)`): the symbol is exported, declared and bound, and the entry's argument checks touch
no device - every check it inherits from `fg_rollout_hd_actor_gru` first, in this entry's name where that entry names itself,
then its own (states_every, rnn_states), while `fg_rollout_hd_actor_gru` answers the same bad calls with its old texts."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest

from formation_gym import _native
from formation_gym.environment import MultiAgentEnv
from formation_gym.vec_env import FormationVecEnv
from tests.actor_testlib import LIB, ROOT, fake_actor as _fake_actor, params as _params
from tests.test_actor_recurrent_cpu import BAD_CALLS, BAD_STATE, _fake_gru, _fake_norm

ENTRY = "fg_rollout_hd_actor_gru_states"
_OLD, _NEW = "fg_rollout_hd_actor_gru: ", ENTRY + ": "


def test_symbol_exported_declared_and_bound():
    assert ENTRY in _native.SIGNATURES
    restype, argtypes = _native.SIGNATURES[ENTRY]
    old = _native.SIGNATURES["fg_rollout_hd_actor_gru"][1]
    # every argument of fg_rollout_hd_actor_gru up to and including rnn_state, then rnn_states, states_every, obs_every, stream
    assert restype is ctypes.c_int
    assert list(argtypes) == list(old[:-2]) + [ctypes.c_void_p, ctypes.c_int] + list(old[-2:])
    assert hasattr(_native.load(), ENTRY)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    assert re.search(r"\bT %s\b" % ENTRY, exported)
    header = open(os.path.join(ROOT, "include", "formation_hip.h")).read()
    decl = re.search(r"\bint %s\(([^;]*)\);" % ENTRY, header)
    assert decl is not None
    names = [a.split()[-1].lstrip("*") for a in decl.group(1).replace("\n", " ").split(",")]
    old_decl = re.search(r"\bint fg_rollout_hd_actor_gru\(([^;]*)\);", header)
    old_names = [a.split()[-1].lstrip("*") for a in old_decl.group(1).replace("\n", " ").split(",")]
    assert names == old_names[:-2] + ["rnn_states", "states_every"] + old_names[-2:]
    assert names[-5:] == ["rnn_state", "rnn_states", "states_every", "obs_every", "stream"]
    assert _native.load().fg_abi_version() == 8                                    # an additive change


def test_keyword_reaches_every_layer():
    for fn in (MultiAgentEnv.rollout_actor, FormationVecEnv.rollout_actor):
        p = inspect.signature(fn).parameters
        assert p["rnn_states_every"].default is None
        assert list(p)[-2:] == ["rnn_state", "rnn_states_every"]


def _call(lib, states, H=64, N=9, K=20, B=128, actor="fake", norm="fake", gru="fake", log_std=4096, logp=4096, rnn_state=4096,
          rnn_states=4096, states_every=5):
    """(status, fg_last_error()) of the entry with stand-in addresses; `states`: the new entry, else fg_rollout_hd_actor_gru
    (which takes neither rnn_states nor states_every)."""
    actor = _fake_actor(H) if actor == "fake" else actor
    norm = _fake_norm() if norm == "fake" else norm if norm is None else _fake_norm(**norm)
    gru = _fake_gru() if gru == "fake" else gru if gru is None else _fake_gru(**gru)
    lead = (_params(), actor, norm, gru, log_std, B, N, K, *([ctypes.c_void_p(4096)] * 12), logp, rnn_state)
    if states:
        rc = lib.fg_rollout_hd_actor_gru_states(*lead, rnn_states, states_every, 1, None)
    else:
        rc = lib.fg_rollout_hd_actor_gru(*lead, 1, None)
    return rc, lib.fg_last_error().decode()


# the entry's own checks, after every inherited one: (what is wrong, status, message after the entry's name)
BAD_STATES = [
    (dict(states_every=0), -1, "states_every >= 1 required"),
    (dict(states_every=-3), -1, "states_every >= 1 required"),
    (dict(rnn_states=None), -1, "rnn_states is NULL"),
    (dict(rnn_states=4104), -3, "rnn_states must be 16-byte aligned"),
    (dict(states_every=0, rnn_states=None), -1, "states_every >= 1 required"),
]


def test_inherited_failures_come_first_in_this_entrys_name():
    lib = _native.load()
    assert any(text.startswith(_OLD) for _, _, text in BAD_CALLS)
    for wrong, status, text in BAD_CALLS + BAD_STATE:
        want = _NEW + text[len(_OLD):] if text.startswith(_OLD) else text
        # ... even with everything of its own wrong as well
        for own in (dict(), dict(states_every=0, rnn_states=None), dict(rnn_states=4104)):
            rc, got = _call(lib, True, **wrong, **own)
            assert rc == status and got == want, (wrong, own, rc, got)
        # the older entry: its old texts
        rc, got = _call(lib, False, **wrong)
        assert rc == status and got == text, (wrong, rc, got)


def test_own_argument_checks():
    lib = _native.load()
    for wrong, status, text in BAD_STATES:
        rc, got = _call(lib, True, **wrong)
        assert rc == status and got == _NEW + text, (wrong, rc, got)
    # a bad buffer of the rollout itself is an inherited check: it is reported before states_every
    lead = (_params(), _fake_actor(64), _fake_norm(), _fake_gru(), 4096, 128, 9, 20)
    bufs = [ctypes.c_void_p(4096)] * 12
    bufs[0] = None
    rc_new = lib.fg_rollout_hd_actor_gru_states(*lead, *bufs, 4096, 4096, 4096, 0, 1, None)
    text_new = lib.fg_last_error().decode()
    rc_old = lib.fg_rollout_hd_actor_gru(*lead, *bufs, 4096, 4096, 1, None)
    assert rc_new == rc_old != 0 and text_new == lib.fg_last_error().decode() and "states_every" not in text_new


def test_empty_batch_returns_ok_without_a_launch():
    lib = _native.load()
    assert _call(lib, True, B=0)[0] == 0
    assert _call(lib, True, B=0, rnn_state=None, rnn_states=None)[0] == 0
    assert _call(lib, True, B=0, log_std=None, logp=4098)[0] == 0
    # the value checks hold at B = 0 too
    assert _call(lib, True, B=0, states_every=0) == (-1, _NEW + "states_every >= 1 required")
    assert _call(lib, True, B=0, rnn_states=4104) == (-3, _NEW + "rnn_states must be 16-byte aligned")


def test_old_entry_ignores_what_it_does_not_take():
    """fg_rollout_hd_actor_gru is the new entry with rnn_states = NULL: no new check reaches it."""
    lib = _native.load()
    assert _call(lib, False, B=0)[0] == 0
    for wrong, status, text in BAD_STATE:
        assert _call(lib, False, **wrong) == (status, text)
