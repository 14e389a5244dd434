"""GPU: a population of policies in one launch, with the fitness formed on the device (bsk_population_*; kernels in
csrc/bsk_policy.hip and csrc/bsk_population.hip; contract in include/bskgpu.h).

Every check is an EQUALITY, against code that already ships or against a numpy restatement - no tolerance is picked anywhere:
  - bsk_population_act against P calls of bsk_policy_act (the two kernels share their device functions), relu and tanh alike;
  - relu networks against mlp_ref / act_ref;
  - bsk_population_rollout against P separate bsk_policy_rollout calls on handles of E envs;
  - the device fitness against bsk_select_branches' values on the recorded histories and against population_fitness_ref.
Shapes: the member rule can go wrong in the workgroup -> member division, at the tail and in the per-member block offset, so
P = 3 / E = 64 (one workgroup per member), P = 2 / E = 128 (two) and P = 5 / E = 64 with a value network; members have distinct
random parameters, so a wrong block cannot pass.
"""
import ctypes
import subprocess

import numpy as np
import pytest

from _device_bits import build_c_consumer, download as _download, same as _same
from _policy_bounds import centred, observation_like, reset_observations, seeded_policy
from basilisk_env_amd import _hip, _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET, FLAG_DESAT, FLAG_DRAG, FLAG_POWER, FLAG_SUN_THIRD_BODY, GRAV_PM_J2, GRAV_SH
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch

pytestmark = pytest.mark.gpu

FULL = FLAG_POWER | FLAG_SUN_THIRD_BODY | FLAG_DRAG | FLAG_DESAT
HIST = (("obs", 40, np.float64, 5), ("reward", 8, np.float64, 1), ("reason", 1, np.uint8, 1), ("action", 4, np.int32, 1),
        ("logp", 4, np.float32, 1), ("value", 4, np.float32, 1))


def _members(n_members, hidden, activation, value_hidden, seed, centre=False):
    """-> (Spec, params (P, n_params)): a seeded network per member, each from a seed of its own"""
    blocks = []
    for m in range(n_members):
        spec, block = seeded_policy(hidden, activation, value_hidden, seed=seed + 17 * m)
        if centre:      # (all three actions occur on the env's observations: a loop under a constant action tests little)
            block = centred(spec, block, reset_observations(sample_ic_batch(500, 4, seed=m), default_config(4, GRAV_PM_J2)))
        blocks.append(block)
    params = np.stack(blocks)
    assert len({b.tobytes() for b in params}) == n_members
    return spec, params


def _envs(p):
    p.sync()
    out = {"state": p.get_state()}
    out["steps"], out["ticks"] = p.get_counters()
    out["obs"], out["rew"], _, out["why"] = p.get_obs()
    v = p.device_views()
    out["done_mask"] = _download(v["done_mask"].__cuda_array_interface__["data"][0], np.uint64, (p.n_envs + 63) // 64)
    if "terminal_obs" in v:
        out["term_obs"], out["episodes"] = p.get_terminal_obs()
    return out


def _member_slice(key, val, m, E):
    """member m's part of one of _envs' arrays of the whole handle"""
    if key == "done_mask":
        return val[m * E // 64:(m + 1) * E // 64]
    return val[..., m * E:(m + 1) * E]


def _propagator(n, ic, flags=0, max_length=None, env_base=0, stream=None, pool_seed=15, warm=1, k=1):
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= flags
    if max_length:
        cfg.max_length = max_length
    p = BatchedPropagator(cfg, n, stream=stream)
    if flags & FLAG_AUTO_RESET:
        p.set_ic_pool(sample_ic_batch(41, 4, seed=pool_seed))
    p.set_env_base(env_base)
    p.reset(ic)
    for _ in range(warm):
        p.step(np.zeros(n, np.int32), k)           # (the observation buffers hold a step's output, not a reset's)
    return p


CASES = [(3, 64, (), None), (2, 128, (16,), None), (5, 64, (32, 16), (16,)), (2, 128, (128, 128, 128), (128, 128, 128))]


@pytest.mark.parametrize("activation", ["relu", "tanh"])
@pytest.mark.parametrize("n_members,E,hidden,value_hidden", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_act_equals_one_policy_launch_per_member_and_the_numpy_chain(n_members, E, hidden, value_hidden, activation):
    import torch
    lib = _lib.load()
    n, pad, base = n_members * E, 37, 1000
    spec, params = _members(n_members, hidden, activation, value_hidden, seed=3)
    obs = observation_like(n, seed=n)
    block = torch.full((5, n + pad), float("nan"), dtype=torch.float64, device="cuda")
    block[:, :n] = torch.from_numpy(obs).cuda()
    pop = P.PolicyPopulation(spec, params)
    singles = [P.DevicePolicy(spec, params[m]) for m in range(n_members)]

    def outputs():
        return {"action": torch.full((n + 64,), -7, dtype=torch.int32, device="cuda"),
                "logp": torch.full((n + 64,), -7.0, dtype=torch.float32, device="cuda"),
                "value": torch.full((n + 64,), -7.0, dtype=torch.float32, device="cuda"),
                "logits": torch.full((3, n + 64), -7.0, dtype=torch.float32, device="cuda")}
    for mode in (0, 1):
        got, want = outputs(), outputs()
        pop.set_rng(9, 5)
        for pol in singles:
            pol.set_rng(9, 5)
        torch.cuda.synchronize()
        vptr = lambda o: o["value"].data_ptr() if value_hidden is not None else None        # noqa: E731
        _lib.check(lib.bsk_population_act(pop._handle(), block.data_ptr(), n + pad, n, E, base, mode, got["action"].data_ptr(),
                                          got["logp"].data_ptr(), vptr(got), got["logits"].data_ptr(), n + 64, None))
        for m, pol in enumerate(singles):
            at = m * E
            _lib.check(lib.bsk_policy_act(pol._handle(), block.data_ptr() + 8 * at, n + pad, E, base + at, mode,
                                          want["action"].data_ptr() + 4 * at, want["logp"].data_ptr() + 4 * at,
                                          want["value"].data_ptr() + 4 * at if value_hidden is not None else None,
                                          want["logits"].data_ptr() + 4 * at, n + 64, None))
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in got.items()}
        want = {k: v.cpu().numpy() for k, v in want.items()}
        for key in got:      # every element, the sentinels beyond n (and a value row nobody asked for) included
            assert _same(got[key], want[key]), (mode, key)
        assert (got["action"][n:] == -7).all() and (got["logits"][:, n:] == -7).all() and (got["logp"][n:] == -7).all()
        assert got["action"][:n].min() >= 0 and got["action"][:n].max() <= 2 and (got["logp"][:n] != -7).all()
        assert (got["value"][:n] != -7).all() if value_hidden is not None else (got["value"] == -7).all()
        assert pop.get_rng() == singles[0].get_rng() == (9, 5 + mode)
        if mode == 1:
            assert len(set(got["action"][:n].tolist())) > 1
        if activation == "relu" and mode == 0:
            for m in range(n_members):       # the definition itself, member by member: a wrong block offset cannot pass
                cols = slice(m * E, (m + 1) * E)
                l, v = P.mlp_ref(spec, params[m], obs[:, cols])
                assert _same(got["logits"][:, cols], l) and np.array_equal(got["action"][cols], P.act_ref(l, "greedy")[0]), m
                if value_hidden is not None:
                    assert _same(got["value"][cols], v), m
    assert bool(torch.isnan(block[:, n:]).all())
    # the binding: the same launch through PolicyPopulation.act on the device array
    res = pop.act(block[:, :n], mode="greedy", want=("logits",))
    pop.sync()
    assert _same(_download(res["logits"].__cuda_array_interface__["data"][0], np.float32, 3 * n).reshape(3, n), want["logits"][:, :n])
    for x in singles + [pop]:
        x.close()


def _rollout_buffers(T, n, n_members):
    import torch
    bufs = {key: torch.zeros(T * n * size, dtype=torch.uint8, device="cuda") for key, size, _, _ in HIST}
    bufs["env_value"] = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    bufs["env_len"] = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    bufs["fitness"] = torch.full((n_members,), -7.0, dtype=torch.float64, device="cuda")
    bufs["mean_len"] = torch.full((n_members,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return bufs


def _hist_host(bufs, T, n, value=True):
    out = {}
    for key, size, dt, rows in HIST:
        if key == "value" and not value:
            continue
        out[key] = bufs[key].cpu().numpy().view(dt).reshape((T, 5, n) if rows == 5 else (T, n))
    for key in ("env_value", "env_len", "fitness", "mean_len"):
        out[key] = bufs[key].cpu().numpy()
    return out


def _population_rollout(pop, prop, T, k, gamma, bufs, mode="greedy", value=True):
    pop.rollout_device(prop, T, k, mode, gamma, *(bufs[key].data_ptr() if key != "value" or value else None for key, _, _, _ in HIST),
                       d_env_value=bufs["env_value"].data_ptr(), d_env_len=bufs["env_len"].data_ptr(),
                       d_fitness=bufs["fitness"].data_ptr(), d_mean_len=bufs["mean_len"].data_ptr())


@pytest.mark.parametrize("n_members,E,gamma", [(3, 64, 0.97), (2, 128, 1.0)])
def test_rollout_equals_separate_rollouts_and_the_fitness_its_definitions(n_members, E, gamma):
    import torch
    lib = _lib.load()
    n, T, k = n_members * E, 26, 1
    spec, params = _members(n_members, (32, 16), "relu", (16,), seed=31, centre=True)
    ic = sample_ic_batch(n, 4, seed=14)
    whole = _propagator(n, ic, FLAG_AUTO_RESET, max_length=7)
    pop = P.PolicyPopulation(spec, params)
    bufs = _rollout_buffers(T, n, n_members)
    _population_rollout(pop, whole, T, k, gamma, bufs)
    # bsk_select_branches on the histories this very rollout recorded: one group per member
    first = torch.zeros(n, dtype=torch.int32, device="cuda")
    values = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    best = torch.zeros(n_members, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(lib.bsk_select_branches(bufs["reward"].data_ptr(), bufs["reason"].data_ptr(), first.data_ptr(), T, n, E, gamma,
                                       values.data_ptr(), None, best.data_ptr(), ctypes.c_void_p(whole.stream_ptr())))
    whole.sync()
    got = _hist_host(bufs, T, n)
    ea = _envs(whole)
    # (1) the same histories and the same handle as P separate rollouts on handles of E envs
    for m in range(n_members):
        cols = slice(m * E, (m + 1) * E)
        part = _propagator(E, ic[:, cols], FLAG_AUTO_RESET, max_length=7, env_base=m * E)
        pol = P.DevicePolicy(spec, params[m])
        want = pol.rollout(part, T, k, "greedy")
        for key in ("obs", "reward", "reason", "action", "logp", "value"):
            assert _same(got[key][..., cols], want[key]), (m, key)
        eb = _envs(part)
        assert set(ea) == set(eb) and "episodes" in ea
        for key in ea:
            assert _same(_member_slice(key, ea[key], m, E), eb[key]), (m, key)
        part.close()
        pol.close()
    assert len(set(got["action"].ravel().tolist())) > 1 and int(ea["episodes"].min()) >= 3
    # (2) the fitness: bsk_select_branches' values, and the numpy restatement of the whole definition
    assert _same(got["env_value"], values.cpu().numpy())
    ref = P.population_fitness_ref(got["reward"], got["reason"], gamma, n_members)
    for key in ("env_value", "env_len", "fitness", "mean_len"):
        assert _same(got[key], ref[key]), key
    # the case is not a trivial one: episodes ended early, the envs restarted and went on earning reward that does not count
    ended = got["env_len"] < T
    assert ended.all() and got["env_len"].min() >= 1
    later = np.array([np.abs(got["reward"][got["env_len"][j]:, j]).sum() for j in range(n)])
    assert (later != 0).any() and (got["reason"] != 0).sum() >= 3 * n
    full = P.population_fitness_ref(got["reward"], np.zeros_like(got["reason"]), gamma, n_members)
    assert not np.array_equal(full["fitness"], got["fitness"])
    # the host convenience forms the same numbers on an identical handle
    again = _propagator(n, ic, FLAG_AUTO_RESET, max_length=7)
    host = pop.evaluate(again, T, k, "greedy", gamma)
    for key in ("env_value", "env_len", "fitness", "mean_len"):
        assert _same(host[key], got[key]), key
    for x in (whole, again, pop):
        x.close()


def test_rollout_full_scenario_at_the_reference_substeps():
    n_members, E, T, k = 2, 64, 2, 1800
    n = n_members * E
    spec, params = _members(n_members, (16,), "relu", None, seed=41, centre=True)
    ic = sample_ic_batch(n, 4, seed=17)
    whole = _propagator(n, ic, FULL, k=k)
    pop = P.PolicyPopulation(spec, params)
    bufs = _rollout_buffers(T, n, n_members)
    _population_rollout(pop, whole, T, k, 0.97, bufs, value=False)
    whole.sync()
    got = _hist_host(bufs, T, n, value=False)
    ea = _envs(whole)
    for m in range(n_members):
        cols = slice(m * E, (m + 1) * E)
        part = _propagator(E, ic[:, cols], FULL, env_base=m * E, k=k)
        pol = P.DevicePolicy(spec, params[m])
        want = pol.rollout(part, T, k, "greedy")
        for key in ("obs", "reward", "reason", "action", "logp"):
            assert _same(got[key][..., cols], want[key]), (m, key)
        eb = _envs(part)
        for key in ea:
            assert _same(_member_slice(key, ea[key], m, E), eb[key]), (m, key)
        part.close()
        pol.close()
    ref = P.population_fitness_ref(got["reward"], got["reason"], 0.97, n_members)
    for key in ("env_value", "env_len", "fitness", "mean_len"):
        assert _same(got[key], ref[key]), key
    whole.close()
    pop.close()


def test_device_parameters_round_trip_and_drive_the_same_rollout():
    import torch
    n_members, E, T, k = 5, 64, 4, 1
    n = n_members * E
    spec, A = _members(n_members, (32, 16), "tanh", (16,), seed=51)
    _, B = _members(n_members, (32, 16), "tanh", (16,), seed=151)
    pop = P.PolicyPopulation(spec, n_members=n_members)
    for m in range(n_members):
        assert not pop.member(m).any()                     # NULL parameters: all-zero members
    d_B = torch.from_numpy(B).cuda()
    torch.cuda.synchronize()
    pop.set_params_device(d_B)                             # (anything with __cuda_array_interface__)
    for m in range(n_members):
        assert _same(pop.member(m), B[m]), m
    ic = sample_ic_batch(n, 4, seed=19)
    runs = []
    for how in ("device", "host"):
        prop = _propagator(n, ic)
        if how == "host":
            pop.set_params(A)                              # (something else in between)
            pop.set_params(B)
        bufs = _rollout_buffers(T, n, n_members)
        _population_rollout(pop, prop, T, k, 0.97, bufs)
        prop.sync()
        runs.append((_hist_host(bufs, T, n), _envs(prop)))
        prop.close()
    for part in (0, 1):
        for key in runs[0][part]:
            assert _same(runs[0][part][key], runs[1][part][key]), key
    # first / count: only the named members change; a raw pointer is taken as it is
    pop.set_params(A)
    pop.set_params_device(d_B[1:3].contiguous().data_ptr(), first=1, count=2)
    for m in range(n_members):
        assert _same(pop.member(m), B[m] if m in (1, 2) else A[m]), m
    pop.set_params_device(d_B[4:], first=4)
    assert _same(pop.member(4), B[4]) and _same(pop.member(3), A[3]) and _same(pop.member(0), A[0])
    # the winner becomes a DevicePolicy: the block get_member returns is the one bsk_policy_create takes
    obs = observation_like(E, seed=2)
    d_obs = torch.from_numpy(obs).cuda()
    pol = P.DevicePolicy(spec, pop.member(2))
    res = pol.act(d_obs, "greedy", ("logits",))
    pol.sync()
    one = _download(res["logits"].__cuda_array_interface__["data"][0], np.float32, 3 * E)
    block = torch.from_numpy(np.tile(obs, (1, n_members))).cuda()
    res = pop.act(block, E, "greedy", ("logits",))
    pop.sync()
    every = _download(res["logits"].__cuda_array_interface__["data"][0], np.float32, 3 * n).reshape(3, n)
    assert _same(every[:, 2 * E:3 * E].ravel(), one)
    with pytest.raises(ValueError):
        pop.set_params_device(d_B[:, ::2])
    with pytest.raises(ValueError):
        pop.set_params_device(d_B.double())
    with pytest.raises(ValueError):
        pop.set_params(B[:3])
    pol.close()
    pop.close()


def test_no_host_traffic_and_replay_from_a_hip_graph():
    import torch
    n_members, E, T, k = 3, 64, 3, 1
    n = n_members * E
    spec, A = _members(n_members, (16,), "relu", None, seed=61, centre=True)
    sets = [A, _members(n_members, (16,), "relu", None, seed=161, centre=True)[1], _members(n_members, (16,), "relu", None, seed=261, centre=True)[1]]
    ic = sample_ic_batch(n, 4, seed=23)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        def make():
            prop = _propagator(n, ic, FLAG_AUTO_RESET, max_length=5, stream=side.cuda_stream)
            pop = P.PolicyPopulation(spec, n_members=n_members)
            d_params = torch.from_numpy(sets[0]).cuda()
            bufs = _rollout_buffers(T, n, n_members)
            return prop, pop, d_params, bufs

        def one(prop, pop, d_params, bufs):
            pop.set_params_device(d_params, stream=side.cuda_stream)
            _population_rollout(pop, prop, T, k, 0.97, bufs, value=False)

        # the reference: the same three generations, never captured
        prop, pop, d_params, bufs = make()
        want = []
        for params in sets:
            d_params.copy_(torch.from_numpy(params))
            one(prop, pop, d_params, bufs)
            prop.sync()
            want.append((_hist_host(bufs, T, n, value=False), _envs(prop)))
        assert not _same(want[1][0]["fitness"], want[2][0]["fitness"])
        prop.close()
        pop.close()

        prop, pop, d_params, bufs = make()
        one(prop, pop, d_params, bufs)                     # the warming call: it allocates the population's scratch rows
        prop.sync()
        c0 = BatchedPropagator.debug_counters()
        d_params.copy_(torch.from_numpy(sets[1]))
        one(prop, pop, d_params, bufs)
        assert BatchedPropagator.debug_counters() == c0    # no copy, no synchronisation
        prop.sync()
        got = (_hist_host(bufs, T, n, value=False), _envs(prop))
        for part in (0, 1):
            for key in want[1][part]:
                assert _same(got[part][key], want[1][part][key]), key
        prop.close()
        pop.close()

        # captured once, replayed twice with new device parameters in between
        prop, pop, d_params, bufs = make()
        one(prop, pop, d_params, bufs)
        prop.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            one(prop, pop, d_params, bufs)
        for g in (1, 2):
            c0 = BatchedPropagator.debug_counters()        # (reading the handle back below copies and synchronises)
            d_params.copy_(torch.from_numpy(sets[g]))
            graph.replay()
            torch.cuda.synchronize()
            assert BatchedPropagator.debug_counters() == c0
            got = (_hist_host(bufs, T, n, value=False), _envs(prop))
            for part in (0, 1):
                for key in want[g][part]:
                    assert _same(got[part][key], want[g][part][key]), (g, key)
        assert int(got[1]["episodes"].sum()) > 0
        prop.close()
        pop.close()


def test_a_first_rollout_that_must_allocate_cannot_be_captured():
    import torch
    n_members, E = 2, 64
    n = n_members * E
    spec, params = _members(n_members, (), "relu", None, seed=71)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        prop = _propagator(n, sample_ic_batch(n, 4, seed=2), stream=side.cuda_stream, warm=0)
        pop = P.PolicyPopulation(spec, params)
        hist = torch.zeros(n, dtype=torch.int32, device="cuda")
        prop.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.BskError) as e:
                pop.rollout_device(prop, 1, 1, d_action_hist=hist.data_ptr())      # (even with an action history: the running values)
            assert e.value.code == -1 and "captured" in str(e.value)
        prop.close()
        pop.close()


def test_refusals_come_before_any_launch():
    import torch
    lib = _lib.load()
    n_members, E = 2, 64
    n = n_members * E
    spec, params = _members(n_members, (16,), "relu", None, seed=91)
    pop = P.PolicyPopulation(spec, params)
    spec_v, params_v = _members(n_members, (16,), "relu", (16,), seed=91)
    pop_v = P.PolicyPopulation(spec_v, params_v)
    obs = torch.from_numpy(observation_like(n)).cuda()
    act = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    f32 = torch.full((3, n), -7.0, dtype=torch.float32, device="cuda")
    f64 = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    fit = torch.full((n_members,), -7.0, dtype=torch.float64, device="cuda")
    d_par = torch.full((n_members * P.n_params(spec),), 3.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    h, o, a, f = pop._handle(), obs.data_ptr(), act.data_ptr(), f32.data_ptr()
    bad = [
        (None, o, n, n, E, 0, 0, a, None, None, None, 0, None),          # no population
        (h, None, n, n, E, 0, 0, a, None, None, None, 0, None),          # no observations
        (h, o, n, n, E, 0, 0, None, None, None, None, 0, None),          # no actions
        (h, o, n, n - 64, E, 0, 0, a, None, None, None, 0, None),        # n != n_members * envs_per_member
        (h, o, n, n, E // 2, 0, 0, a, None, None, None, 0, None),        # ... either way
        (h, o, 96, 96, 48, 0, 0, a, None, None, None, 0, None),          # envs_per_member no multiple of 64
        (h, o, n, n, 0, 0, 0, a, None, None, None, 0, None),
        (h, o, n - 1, n, E, 0, 0, a, None, None, None, 0, None),         # rows closer than n
        (h, o, n, n, E, -1, 0, a, None, None, None, 0, None),            # negative env_base
        (h, o, n, n, E, 0, 2, a, None, None, None, 0, None),             # bad mode
        (h, o, n, n, E, 0, 0, a, None, f, None, 0, None),                # value output without a value network
        (h, o, n, n, E, 0, 0, a, None, None, f, n - 1, None),            # logits rows closer than n
    ]
    for args in bad:
        assert lib.bsk_population_act(*args) == -1, args
        assert lib.bsk_last_error()
    # first / count out of range, NULL parameters
    for args in ((h, d_par.data_ptr(), -1, 1), (h, d_par.data_ptr(), 0, 0), (h, d_par.data_ptr(), 0, 3), (h, d_par.data_ptr(), 2, 1),
                 (h, d_par.data_ptr(), 1, 2), (h, None, 0, 1), (None, d_par.data_ptr(), 0, 1)):
        assert lib.bsk_population_set_params_device(*args, None) == -1, args
    p1 = np.empty(P.n_params(spec), np.float32)
    assert lib.bsk_population_get_member(h, 2, p1.ctypes.data) == -1 and lib.bsk_population_get_member(h, -1, p1.ctypes.data) == -1
    assert lib.bsk_population_get_member(h, 0, None) == -1 and lib.bsk_population_set_params(h, None) == -1
    torch.cuda.synchronize()
    assert bool((act == -7).all()) and bool((f32 == -7).all())       # nothing was launched
    for m in range(n_members):
        assert _same(pop.member(m), params[m])
    # rollout
    prop = _propagator(n, sample_ic_batch(n, 4, seed=4))
    odd = _propagator(n + 64, sample_ic_batch(n + 64, 4, seed=4))       # three workgroups for two members
    small = _propagator(64, sample_ic_batch(64, 4, seed=4))             # 32 envs per member
    cfg = default_config(4, GRAV_SH)
    cfg.sh_degree = 8
    no_sh = BatchedPropagator(cfg, n)                                   # harmonics asked for, never set
    no_sh.reset(sample_ic_batch(n, 4, seed=4))
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    no_pool = BatchedPropagator(cfg, n)                                 # auto-reset without a pool
    no_pool.reset(sample_ic_batch(n, 4, seed=4))
    props = (prop, odd, small, no_sh, no_pool)
    before = [_envs(p) for p in props]
    c0 = BatchedPropagator.debug_counters()
    hp = prop._handle()
    tail = (None, None, None, a, None, None, f64.data_ptr(), None, fit.data_ptr(), None)
    for args in ((None, hp, 0, 1, 1, 1.0), (h, None, 0, 1, 1, 1.0), (h, hp, 0, 0, 1, 1.0), (h, hp, 0, 1, 0, 1.0), (h, hp, 3, 1, 1, 1.0),
                 (h, hp, 0, 1, 1, float("nan")), (h, hp, 0, 1, 1, float("inf")), (h, hp, 0, 1, 1, -float("inf")),
                 (h, odd._handle(), 0, 1, 1, 1.0), (h, small._handle(), 0, 1, 1, 1.0), (h, no_sh._handle(), 0, 1, 1, 1.0),
                 (h, no_pool._handle(), 0, 1, 1, 1.0)):
        assert lib.bsk_population_rollout(*args, *tail) == -1, args
        assert lib.bsk_last_error()
    value_tail = (None, None, None, a, None, f, f64.data_ptr(), None, fit.data_ptr(), None)
    assert lib.bsk_population_rollout(h, hp, 0, 1, 1, 1.0, *value_tail) == -1          # a value history without a value network
    assert b"value network" in lib.bsk_last_error()
    assert BatchedPropagator.debug_counters() == c0
    torch.cuda.synchronize()
    assert bool((act == -7).all()) and bool((f32 == -7).all()) and bool((f64 == -7).all()) and bool((fit == -7).all())
    for p, was in zip(props, before):
        now = _envs(p)
        for key in was:
            assert _same(was[key], now[key]), key
    # a population and a handle on different devices
    if _hip.device_count() > 1:
        other = P.PolicyPopulation(spec, params, device=1)
        assert lib.bsk_population_rollout(other._handle(), hp, 0, 1, 1, 1.0, *([None] * 10)) == -1
        assert b"different devices" in lib.bsk_last_error()
        other.close()
    with pytest.raises(_lib.BskGpuUnavailable):
        P.PolicyPopulation(spec, params, device=_hip.device_count())
    # ... and the same calls with legal arguments do run
    assert lib.bsk_population_rollout(pop_v._handle(), hp, 0, 1, 1, 1.0, *value_tail) == 0
    prop.sync()
    assert bool((act != -7).all()) and bool((f32.ravel()[:n] != -7).all()) and bool((f64 != -7).all()) and bool((fit != -7).all())
    with pytest.raises(ValueError):
        pop.act(prop, want=("value",))
    with pytest.raises(ValueError):
        pop.rollout_device(prop, 1, 1, "softmax")
    for x in props + (pop, pop_v):
        x.close()


def test_two_evolution_strategy_generations_are_reproducible():
    n_members, E, T, k = 4, 64, 8, 1
    n = n_members * E
    spec, theta0 = seeded_policy((16,), "tanh", None, seed=5)
    ic = sample_ic_batch(n, 4, seed=29)

    def run():
        es = P.EvolutionStrategy(theta0, n_members, sigma=0.1, lr=0.05, seed=3)
        pop = P.PolicyPopulation(spec, n_members=n_members)
        out = []
        for _ in range(2):
            members = es.ask()
            pop.set_params(members)
            prop = _propagator(n, ic, FLAG_AUTO_RESET, max_length=6)
            res = pop.evaluate(prop, T, k, "greedy", 0.99)
            prop.close()
            es.tell(res["fitness"])
            out.append((members, res["fitness"], res["mean_len"]))
        pop.close()
        return out, es.theta
    a, theta_a = run()
    b, theta_b = run()
    for (ma, fa, la), (mb, fb, lb) in zip(a, b):
        assert _same(ma, mb) and _same(fa, fb) and _same(la, lb)
        assert np.isfinite(fa).all() and fa.shape == (n_members,) and (la >= 1).all() and (la <= T).all()
    assert _same(theta_a, theta_b) and not _same(a[0][0], a[1][0])          # (the second generation asks other members)
    assert _same(theta_a[:10], theta0[:10].astype(np.float64))             # in_scale / in_shift never move


def test_c_consumer_prints_the_python_bindings_fitness(tmp_path):
    """tests/c_abi/c_abi_population.c: bsk_population_create / _rollout / _set_params_device from plain C99; its printout equals the
    Python binding's"""
    exe = build_c_consumer(tmp_path, "c_abi_population")
    n_members, E = 3, 64
    n = n_members * E
    ic = sample_ic_batch(n, 4, seed=53)
    spec, params = _members(n_members, (16,), "relu", None, seed=97, centre=True)
    ic.tofile(tmp_path / "ic.bin")
    params.tofile(tmp_path / "params.bin")
    got = subprocess.check_output([str(exe), str(tmp_path / "ic.bin"), str(n), str(tmp_path / "params.bin"), str(n_members)]).decode().split()
    assert len(got) == 4 * n_members
    pop = P.PolicyPopulation(spec, params)
    want = []
    for members in (params, np.roll(params, -1, axis=0)):
        pop.set_params(members)
        prop = BatchedPropagator(default_config(4, GRAV_PM_J2), n)
        prop.reset(ic)
        prop.step(np.zeros(n, np.int32), 5)
        res = pop.evaluate(prop, 6, 5, "greedy", 0.97)
        want += res["fitness"].tolist() + res["mean_len"].tolist()
        prop.close()
    pop.close()
    assert [float(v) for v in got] == want
    assert want[:n_members] != want[2 * n_members:3 * n_members]
