"""CPU checks of what a bound launch reads by address and must therefore keep alive and key on:

* `FusedActor.tensors()` / `binding_key()` against the ctypes structs `_native.actor_structs` builds from the same record, for
  every actor family `resolve_actor` can return (N = 3, H = 32);
* the tensors `World.native_params` and formation_hd_env's `params` write into FgParams by address (the per-agent table, the
  device RNG counter, the communication state) live as long as the struct does.
No device: the records and structs are built on CPU tensors, and nothing is launched."""
import ctypes
import gc
import weakref

import pytest
import torch

from formation_gym import _native
from formation_gym.actor_rollout import (GaussianActor, InputBatchNorm, OUNoiseActor, PerAgentActor, RecurrentActor,
                                         resolve_actor)
from formation_gym.core import Agent, World

nn = torch.nn
N, H, D = 3, 32, 18


def _mlp(lead=None, norms=False, head=True):
    mods = [] if lead is None else [lead]
    mods += [nn.Linear(D, H), nn.ReLU()] + ([nn.LayerNorm(H)] if norms else [])
    mods += [nn.Linear(H, H), nn.ReLU()] + ([nn.LayerNorm(H)] if norms else [])
    return nn.Sequential(*(mods + ([nn.Linear(H, 2), nn.Tanh()] if head else [])))


def _gru():
    return RecurrentActor(_mlp(nn.LayerNorm(D), norms=True, head=False), nn.GRUCell(H, H), nn.LayerNorm(H), nn.Linear(H, 2))


FAMILIES = {
    "shared": _mlp,
    "gaussian": lambda: GaussianActor(_mlp()),
    "per_agent": lambda: PerAgentActor([_mlp() for _ in range(N)]),
    "gaussian_per_agent": lambda: GaussianActor(PerAgentActor([_mlp() for _ in range(N)])),
    "layernorm": lambda: _mlp(norms=True),
    "layernorm_input": lambda: _mlp(nn.LayerNorm(D), norms=True),
    "gru": _gru,
    "gaussian_gru": lambda: GaussianActor(_gru()),
    "batchnorm": lambda: _mlp(InputBatchNorm(D)).eval(),
    "batchnorm_per_agent": lambda: PerAgentActor([_mlp(nn.BatchNorm1d(D)) for _ in range(N)]).eval(),
    "ou": lambda: OUNoiseActor(_mlp()),
    "ou_batchnorm": lambda: OUNoiseActor(_mlp(InputBatchNorm(D)).eval()),
}


def _struct_pointers(structs):
    """The non-NULL values of every pointer field of the structs (arrays element by element)."""
    found = set()
    for s in structs:
        for item in ([] if s is None else list(s) if isinstance(s, ctypes.Array) else [s]):
            found |= {getattr(item, name) for name, kind in item._fields_ if kind is ctypes.c_void_p}
    return found - {None}


def _read_in_place(actor):
    """(owner module, attribute, tensor) of every parameter and buffer a launch reads: all but BatchNorm's batch counter."""
    named = list(actor.named_parameters()) + list(actor.named_buffers())
    return [(actor.get_submodule(name.rpartition(".")[0]), name.rpartition(".")[2], t) for name, t in named
            if not name.endswith("num_batches_tracked")]


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_fused_actor_states_once_what_its_launch_reads(family):
    """The structs' pointer fields, with the log_std argument (a pointer of its own in every entry, not a struct field), are
    exactly `tensors()`; those are exactly the module's parameters and buffers; and `binding_key()` is stable for an unchanged
    module and changes when any one of them is re-allocated."""
    torch.manual_seed(0)
    actor = FAMILIES[family]()
    fused = resolve_actor(actor, N)
    assert fused is not None, "every family here has a fused launch"
    held = {t.data_ptr() for t in fused.tensors()}
    assert len(held) == len(fused.tensors())
    assert _struct_pointers(_native.actor_structs(fused)) | {_native.ptr(t) for t in [fused.log_std] if t is not None} == held
    owned = _read_in_place(actor)
    assert {t.data_ptr() for _, _, t in owned} == held
    key = fused.binding_key()
    assert resolve_actor(actor, N).binding_key() == key
    hash(key)
    for mod, attr, t in owned:
        fresh = t.detach().clone()
        setattr(mod, attr, nn.Parameter(fresh) if isinstance(t, nn.Parameter) else fresh)
        again = resolve_actor(actor, N)
        assert again is not None and again.binding_key() != key, "%s.%s re-allocated, same key" % (type(mod).__name__, attr)
        setattr(mod, attr, t)
    assert resolve_actor(actor, N).binding_key() == key


def test_binding_key_tells_eps_and_the_ou_module_apart():
    """What the structs hold by value: every eps; and the OUNoiseActor itself, whose scalars each launch reads from it."""
    torch.manual_seed(0)
    for actor, norm_of in ((_mlp(norms=True), lambda a: a[2]), (_gru(), lambda a: a.norm),
                           (_mlp(InputBatchNorm(D)).eval(), lambda a: a[0])):
        key = resolve_actor(actor, N).binding_key()
        norm_of(actor).eps = 1e-3
        assert resolve_actor(actor, N).binding_key() != key
    inner = _mlp()
    assert resolve_actor(OUNoiseActor(inner), N).binding_key() != resolve_actor(inner, N).binding_key()
    a, b = OUNoiseActor(inner), OUNoiseActor(inner)
    assert resolve_actor(a, N).binding_key() != resolve_actor(b, N).binding_key()


def _world(**agent1):
    world = World(num_envs=4, device="cpu")
    world.dim_c = 2
    world.agents = [Agent() for _ in range(N)]
    for k, v in agent1.items():
        setattr(world.agents[1], k, v)
    return world


def _alive_exactly_with(make, drop):
    """`make()` returns (struct, tensor) after the world has let go of the tensor through `drop`: the tensor lives while the
    struct does, and no longer."""
    p, t = make()
    ref = weakref.ref(t)
    del t
    drop()
    gc.collect()
    assert ref() is not None, "FgParams holds the address of a tensor nobody keeps"
    del p
    gc.collect()
    assert ref() is None


def test_fg_params_pins_the_tensors_it_holds_by_address():
    world = _world(initial_mass=2.0)                                # heterogeneous agents: a per-agent table

    def props():
        p = world.native_params()
        assert p.agent_props == world._props[1].data_ptr()
        return p, world._props[1]
    _alive_exactly_with(props, lambda: setattr(world, "_props", None))

    world = _world()
    world.rng_counter = torch.zeros(1, dtype=torch.int64)

    def counter():
        p = world.native_params()
        assert p.rng_offset_dev == world.rng_counter.data_ptr() and not p.agent_props
        return p, world.rng_counter
    _alive_exactly_with(counter, lambda: setattr(world, "rng_counter", None))

    from formation_gym.envs.formation_hd_env import Scenario
    world, scenario = _world(silent=False), Scenario()
    scenario._seed = 1

    def comm():
        p = scenario.params(world)
        assert p.comm_state == world.comm_c.data_ptr()
        return p, world.comm_c
    _alive_exactly_with(comm, lambda: setattr(world, "comm_c", None))
