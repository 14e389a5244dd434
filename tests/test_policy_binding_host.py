"""CPU: what the three ctypes bindings of basilisk_env_amd/policy.py - DevicePolicy, PolicyPopulation, DeviceEvolutionStrategy - ask of
the C library and the HIP runtime, call by call, held against a recorded log (tests/golden/policy_binding_calls.json).

The library, the device allocator and the runtime are replaced by fakes that record every call with its arguments and return 0;
a fixed script then drives every method of the three classes, good arguments and bad ones.  Scalars are recorded as values; a pointer
as None, as the name of what it points to where the fake handed it out (a handle, a device buffer, a stream: "buf#7" in one call and
in a later one is the same buffer), as the element type, count and CRC-32 of the host array it has to point to where the ABI fixes
that, and as "ptr" otherwise.  The log, the (type, message) of every exception the script provokes and the module's public names
were recorded from the binding as it stood before it was split into policy_spec / policy_ref / policy and given one base class:
    PYTHONPATH=. python tests/test_policy_binding_host.py --record
writes them anew - which is right only when the sequence of C calls is MEANT to change."""
import json
import os
import types
import zlib

import numpy as np
import pytest

from _binding_fakes import FakeArray, FakePropagator, Recorder, _block
from basilisk_env_amd import _hip, _lib
from basilisk_env_amd import policy as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "policy_binding_calls.json")


def _views(rec, res, objs):
    """the dict ``act`` returns -> what each view points to, keeps alive and waits for"""
    def who(x):
        for name, o in objs.items():
            if x is o:
                return name
        return type(x).__name__
    out = {}
    for key, v in res.items():
        a, owner = v.__cuda_array_interface__, v._owner
        out[key] = {"ptr": rec.name_of(a["data"][0]), "shape": list(a["shape"]), "typestr": a["typestr"], "strides": a["strides"],
                    "device": v._device, "stream": rec.names.get(v._stream, v._stream),
                    "owner": ["_ViewOwner", who(owner.policy), who(owner.prop)] if isinstance(owner, P._ViewOwner) else who(owner)}
    rec.log.append(["views", list(res), out])


def _host_arrays(rec, res):
    rec.log.append(["host", [[k, a.dtype.str, list(a.shape)] for k, a in res.items()]])


def run_script(patch):
    """Drives the three classes over the fakes; ``patch(object, name, value)`` is pytest's ``monkeypatch.setattr``."""
    rec = Recorder()
    patch(_lib, "load", lambda: rec.lib)
    patch(_hip, "DeviceBuffer", rec.DeviceBuffer)
    patch(_hip, "runtime", lambda: rec.rt)
    note, raises = rec.note, rec.raises
    spec = P.check_spec((16,), "relu")
    spec_v = P.check_spec((16,), "tanh", (32,), "relu")
    n, n_v = P.n_params(spec), P.n_params(spec_v)

    # ------------------------------------------------------------------------------------------------------------- DevicePolicy
    note("DevicePolicy")
    rec.sizes = {"np": n_v}
    raises(P.DevicePolicy, spec_v, _block(n_v - 1))
    pol = P.DevicePolicy(spec_v, _block(n_v, np.float64))          # (cast to float32 on the way in)
    rec.sizes = {"np": n}
    pol0 = P.DevicePolicy(((16,), "relu"), list(_block(n, at=3.0)), device=0)
    prop = FakePropagator(rec, 128, 0, env_base=4096)
    other = FakePropagator(rec, 64, 1)
    objs = {"pol": pol, "pol0": pol0, "prop": prop}
    note("set_params")
    pol0.set_params(_block(n, np.float64, 1.0).reshape(1, n))
    raises(pol0.set_params, _block(n + 1))
    rec.sizes = {"np": n_v}
    pol.set_params(_block(n_v, at=2.0))
    note("rng")
    pol.set_rng(5)
    pol.set_rng(seed=(1 << 40) + 1, draw=9)
    rec.log.append(["get_rng", list(pol.get_rng())])
    note("sync")
    pol.sync()
    note("act")
    for want in ((), ("logp",), ("value",), ("logits",), ("logits", "value", "logp")):
        _views(rec, pol.act(prop, "greedy", want), objs)
    _views(rec, pol.act(prop), objs)
    _views(rec, pol.act(types.SimpleNamespace(propagator=prop), "sample", ("logp",), env_base=3, stream=rec.pointer("stream")), objs)
    arr = FakeArray(rec.pointer("obs"), (5, 100), "<f8", with_strides=False)
    _views(rec, pol.act(arr, "sample"), objs)
    rec.log.append(["source kept", pol._source is arr])
    arr = FakeArray(rec.pointer("obs"), (5, 300), "<f8", (8 * 333, 8))                  # (more than before: the buffers grow)
    _views(rec, pol.act(arr, want=("value",), env_base=17, stream=rec.pointer("stream")), objs)
    _views(rec, pol0.act(prop, "greedy", ("logp", "logits")), objs)
    raises(pol.act, prop, "softmax")
    raises(pol.act, prop, "greedy", ("entropy",))
    raises(pol0.act, prop, "greedy", ("value",))
    raises(pol.act, other)
    raises(pol.act, np.zeros((5, 4)))
    raises(pol.act, FakeArray(1, (5, 4), "<f4"))
    raises(pol.act, FakeArray(1, (4, 4), "<f8"))
    raises(pol.act, FakeArray(1, (5, 4), "<f8", (32, 16)))
    raises(pol.act, FakeArray(1, (5, 4), "<f8", (24, 8)))
    note("enqueue")
    out = pol.enqueue(prop._obs, 192, 128, "sample", ("logp", "value"), 5, prop._stream)
    rec.log.append(["enqueue ->", {k: rec.name_of(b.ptr) for k, b in out.items()}])
    pol.enqueue(prop._obs, 192, 64)
    raises(pol.enqueue, prop._obs, 192, 64, "best")
    note("rollout_device")
    pol.rollout_device(prop, 3, 2)
    hist = [rec.pointer("hist") for _ in range(6)]
    pol.rollout_device(types.SimpleNamespace(propagator=prop), 4, 1, "sample", *hist)
    pol.rollout_device(prop, 4, 1, d_reward_hist=hist[1], d_value_hist=hist[5])
    raises(pol.rollout_device, prop, 3, 2, "best")
    note("rollout")
    _host_arrays(rec, pol.rollout(prop, 3, 2))
    _host_arrays(rec, pol0.rollout(types.SimpleNamespace(propagator=prop), 2, 1, "sample"))
    rec.fail_next = "bsk_policy_rollout"
    raises(pol.rollout, prop, 3, 2)
    raises(pol.rollout, prop, 3, 2, "best")
    note("close")
    pol.close()
    rec.log.append(["after close", pol._out is None, pol._source is None])
    pol.close()
    pol0.close()
    pol0.close()
    raises(pol.set_rng, 1)
    raises(pol.get_rng)
    raises(pol.set_params, _block(n_v))
    raises(pol.act, prop)
    raises(pol.rollout_device, prop, 1, 1)
    pol.close()

    # --------------------------------------------------------------------------------------------------------- PolicyPopulation
    note("PolicyPopulation")
    members = 4
    rec.sizes = {"np": n, "Pnp": members * n}
    raises(P.PolicyPopulation, spec)
    raises(P.PolicyPopulation, spec, _block(n))
    raises(P.PolicyPopulation, spec, _block(members * (n + 1)).reshape(members, n + 1))
    raises(P.PolicyPopulation, spec, _block(members * n).reshape(members, n), n_members=3)
    pop = P.PolicyPopulation(spec, n_members=members, device=1)
    rec.sizes = {"np": n_v, "Pnp": 2 * n_v}
    pop_v = P.PolicyPopulation(spec_v, _block(2 * n_v, np.float64).reshape(2, n_v), n_members=2)
    rec.sizes = {"np": n, "Pnp": members * n}
    prop1 = FakePropagator(rec, 256, 1)
    objs = {"pop": pop, "pop_v": pop_v, "prop": prop, "prop1": prop1}
    note("set_params")
    pop.set_params(_block(members * n, np.float64, 1.0).reshape(members, n))
    raises(pop.set_params, _block(3 * n).reshape(3, n))
    raises(pop.set_params, _block(members * n))
    note("set_params_device")
    src = rec.pointer("params")
    pop.set_params_device(src)
    pop.set_params_device(src, first=1)
    pop.set_params_device(src, 1, 2, rec.pointer("stream"))
    pop.set_params_device(None, 0, 1)
    arr = FakeArray(src, (members, n), "<f4")
    pop.set_params_device(arr)
    rec.log.append(["source kept", pop._source is arr])
    pop.set_params_device(FakeArray(src, (2 * n,), "<f4", (4,)), first=2, stream=prop1._stream)
    pop.set_params_device(FakeArray(src, (2, n), "<f4", (4 * n, 4), ), 1, 2)
    pop.set_params_device(FakeArray(src, (3 * n,), "<f4", with_strides=False), count=3)
    raises(pop.set_params_device, FakeArray(src, (2, n), "<f8"))
    raises(pop.set_params_device, FakeArray(src, (n + 1,), "<f4"))
    raises(pop.set_params_device, FakeArray(src, (0,), "<f4"))
    raises(pop.set_params_device, FakeArray(src, (2, n), "<f4", (8 * n, 4)))
    raises(pop.set_params_device, FakeArray(src, (2, n), "<f4"), count=3)
    note("member")
    m = pop.member(2)
    rec.log.append(["member ->", m.dtype.str, list(m.shape), "%08x" % zlib.crc32(m.tobytes())])
    note("rng")
    pop.set_rng(7, 8)
    pop.set_rng(seed=3)
    rec.log.append(["get_rng", list(pop.get_rng())])
    note("sync")
    pop.sync()
    note("act")
    for want in ((), ("logp",), ("logits", "logp")):
        _views(rec, pop.act(prop1, None, "greedy", want), objs)
    _views(rec, pop.act(prop1, 32, "sample", ("logp",), env_base=6, stream=rec.pointer("stream")), objs)
    arr = FakeArray(rec.pointer("obs"), (5, 512), "<f8", (8 * 512, 8))
    _views(rec, pop.act(arr, mode="sample", want=("logits",)), objs)
    rec.log.append(["source kept", pop._source is arr])
    _views(rec, pop_v.act(prop, want=("value", "logp")), objs)
    _views(rec, pop_v.act(prop), objs)
    raises(pop.act, prop1, None, "softmax")
    raises(pop.act, prop1, None, "greedy", ("entropy",))
    raises(pop.act, prop1, None, "greedy", ("value",))
    raises(pop.act, prop)
    raises(pop.act, [1.0])
    note("rollout_device")
    pop.rollout_device(prop1, 3, 2)
    hist = [rec.pointer("hist") for _ in range(10)]
    pop.rollout_device(types.SimpleNamespace(propagator=prop1), 4, 1, "sample", 0.97, *hist)
    pop.rollout_device(prop1, 4, 1, gamma=1, d_fitness=hist[8], d_env_len=hist[7])
    raises(pop.rollout_device, prop1, 3, 2, "best")
    note("evaluate")
    _host_arrays(rec, pop.evaluate(prop1, 3, 2))
    _host_arrays(rec, pop_v.evaluate(types.SimpleNamespace(propagator=prop), 2, 1, "sample", 0.5))
    rec.fail_next = "bsk_population_rollout"
    raises(pop.evaluate, prop1, 3, 2)
    raises(pop.evaluate, prop1, 3, 2, "best")

    # -------------------------------------------------------------------------------------------------- DeviceEvolutionStrategy
    note("DeviceEvolutionStrategy")
    raises(P.DeviceEvolutionStrategy, spec, None, members, optimizer="rmsprop")
    raises(P.DeviceEvolutionStrategy, spec, None, members, optimizer="adam", beta1=1.0)
    raises(P.DeviceEvolutionStrategy, spec, _block(n + 2), members)
    es = P.DeviceEvolutionStrategy(spec, None, members, device=1)
    es_a = P.DeviceEvolutionStrategy(spec, _block(n, np.float64, 0.5), members, sigma=0.25, lr=0.125, seed=99, frozen=12, device=1,
                                     optimizer="adam", beta1=0.5, beta2=0.75, eps=0.001, weight_decay=0.0625)
    rec.log.append(["attributes", es.optimizer, list(es.adam), es_a.optimizer, list(es_a.adam), es_a.population, es_a.sigma, es_a.lr,
                    es_a.frozen, es_a.seed, es_a.device, es_a.n_params])
    note("state")
    t = es_a.theta
    rec.log.append(["theta ->", t.dtype.str, list(t.shape), "%08x" % zlib.crc32(t.tobytes()), "generation ->", es_a.generation])
    es_a.set_state()
    es_a.set_state(_block(n, np.float32, 2.0), 6)
    es_a.set_state(generation=3)
    raises(es_a.set_state, _block(n - 1))
    rec.log.append(["generation_ptr ->", rec.name_of(es_a.generation_ptr())])
    note("optimizer")
    es.set_optimizer("adam")
    es.set_optimizer("adam", 0.5, 0.75, 1, 0)
    es.set_optimizer("sgd", beta1=7)
    rec.log.append(["attributes", es.optimizer, list(es.adam)])
    raises(es.set_optimizer, "rmsprop")
    raises(es.set_optimizer, "adam", eps=0.0)
    raises(es.set_optimizer, "adam", weight_decay=-1.0)
    note("moments")
    rec.log.append(["moments ->", [[a.dtype.str, list(a.shape), "%08x" % zlib.crc32(a.tobytes())] for a in es_a.moments]])
    es_a.set_moments()
    es_a.set_moments(_block(n, np.float32), None, [0.5, 0.25])
    es_a.set_moments(v=_block(n, at=1.0))
    raises(es_a.set_moments, _block(n + 1))
    raises(es_a.set_moments, beta_pow=[0.5])
    note("ask / tell")
    es.ask(pop)
    es.ask(pop, prop1._stream)
    fit = rec.pointer("fitness")
    es.tell(fit)
    es.tell(fit, prop1._stream)
    es.tell(None)
    arr = FakeArray(fit, (members,), "<f8", (8,))
    es.tell(arr, stream=prop1._stream)
    rec.log.append(["source kept", es._source is arr])
    es.tell(FakeArray(fit, (members,), "<f8", with_strides=False))
    es.tell(FakeArray(fit, (2, 2), "<f8", (32, 8)))                  # (only a 1-D array's stride is looked at)
    raises(es.tell, FakeArray(fit, (members,), "<f4"))
    raises(es.tell, FakeArray(fit, (members + 1,), "<f8"))
    raises(es.tell, FakeArray(fit, (members,), "<f8", (16,)))
    raises(es.ask, pol)                                              # (a closed policy's handle)
    note("run_generation")
    for reset in (True, False):
        for shared in (False, True):
            es.run_generation(prop1, pop, 5, 2, reset=reset, shared_episodes=shared)
    es_a.run_generation(types.SimpleNamespace(propagator=prop1), pop, 3, 1, "sample", 0.9)
    rec.log.append(["fitness_buffer", rec.name_of(es.fitness_buffer().ptr), rec.name_of(es_a.fitness_buffer().ptr)])

    note("close")
    for obj in (pop, pop_v, es, es_a):
        obj.close()
        obj.close()
    rec.log.append(["after close", pop._out is None, pop._source is None, es.__dict__.get("_fitness") is None, es._source is None])
    raises(pop.set_rng, 1)
    raises(pop.get_rng)
    raises(pop.member, 0)
    raises(pop.set_params_device, src)
    raises(pop.rollout_device, prop1, 1, 1)
    raises(pop.act, prop1)
    raises(es.ask, pop)
    raises(es.tell, fit)
    raises(es.generation_ptr)
    raises(es.set_state)
    raises(lambda: es.theta)
    raises(lambda: es_a.moments)
    for obj in (pop, es):
        obj.close()
    return rec.log, rec.errors


def public_names():
    """what ``from basilisk_env_amd import policy as P`` offers: no modules, and nothing that merely came along from a library"""
    names = []
    for name in dir(P):
        obj = getattr(P, name)
        if name.startswith("_") or isinstance(obj, types.ModuleType):
            continue
        if not getattr(obj, "__module__", "basilisk_env_amd").startswith("basilisk_env_amd"):
            continue
        names.append(name)
    return sorted(names)


def test_the_bindings_make_the_recorded_calls(monkeypatch):
    golden = json.load(open(GOLDEN))
    log, errors = run_script(monkeypatch.setattr)
    log, errors = json.loads(json.dumps(log)), json.loads(json.dumps(errors))
    assert errors == golden["exceptions"]
    for k, (got, want) in enumerate(zip(log, golden["calls"])):
        assert got == want, "entry %d: %r, recorded %r" % (k, got, want)
    assert len(log) == len(golden["calls"])
    for text in ("policy is closed", "population is closed", "evolution strategy is closed"):
        assert ["RuntimeError", text] in errors
    destroyed = [row[1] for row in log if row[0].endswith("_destroy")]
    assert len(destroyed) == len(set(destroyed)) == 6                 # every object once, however often it was closed


def test_every_recorded_public_name_is_still_there():
    golden = json.load(open(GOLDEN))
    missing = sorted(set(golden["public_names"]) - set(public_names()))
    assert not missing, missing
    for name in ("mlp_ref", "check_spec", "es_tell_adam_ref", "EvolutionStrategy", "DevicePolicy", "PolicyPopulation", "DeviceEvolutionStrategy"):
        assert name in golden["public_names"]


if __name__ == "__main__":
    import sys
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: PYTHONPATH=. python tests/test_policy_binding_host.py --record")
    with pytest.MonkeyPatch.context() as mp:
        calls, exceptions = run_script(mp.setattr)
    with open(GOLDEN, "w") as f:
        rows = lambda items: "[\n" + ",\n".join(json.dumps(x) for x in items) + "\n]"      # noqa: E731 - one entry per line
        f.write('{"calls": %s,\n"exceptions": %s,\n"public_names": %s}\n' % (rows(calls), rows(exceptions), json.dumps(public_names())))
    print("%d calls, %d exceptions -> %s" % (len(calls), len(exceptions), GOLDEN))
