"""CPU: the device-free part of the population feature (basilisk_env_amd/policy.py, bsk_population_* in include/bskgpu.h).

``population_fitness_ref`` - the numpy restatement the GPU tests hold the device fitness to - is itself held to a plain Python
double loop that follows the header's text operation by operation; the C-ABI's refusals that need no device; the parameter block
round trip; the evolution strategy on a quadratic; and the plain-C consumer compiles from the header alone.  The scenario of
tests/test_gpu_population_shapes.py (tests/_population_cases.py) runs on the CPU oracle first: what its staggering, constants and
seeds produce - every member mixed, a reordered sum visible, NaN values in a first and in a later trip, a champion past member 64 -
is known before a GPU is.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _population_cases as C
from _oracle_backend import OraclePropagator
from _policy_bounds import seeded_policy
from basilisk_env_amd import _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fitness_loops(reward, reason, gamma, n_members):
    """include/bskgpu.h, word for word, on Python floats (IEEE doubles: every operation rounds on its own)"""
    T, n = len(reward), len(reward[0])
    E = n // n_members
    value, length = [], []
    for j in range(n):
        v, g, ln, alive = 0.0, 1.0, 0, True
        for t in range(T):
            if not alive:
                break
            v = v + g * float(reward[t][j])
            ln += 1
            g = g * gamma
            if reason[t][j] != 0:
                alive = False
        value.append(v)
        length.append(ln)

    def mean(x, m):
        s = [x[m * E + l] for l in range(64)]
        for i in range(1, E // 64):
            for l in range(64):
                s[l] = s[l] + x[m * E + l + 64 * i]
        for stride in (32, 16, 8, 4, 2, 1):
            for l in range(stride):
                s[l] = s[l] + s[l + stride]
        return s[0] / E
    return (value, length, [mean(value, m) for m in range(n_members)], [mean([float(x) for x in length], m) for m in range(n_members)])


def _same(a, b):
    """equal bit for bit (NaN equals NaN; +0.0 and -0.0 differ)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("E,n_members", [(64, 3), (192, 2), (64, 1), (320, 3), (1024, 2)])
@pytest.mark.parametrize("gamma", [1.0, 0.97])
def test_fitness_ref_equals_the_definition_in_plain_loops(E, n_members, gamma):
    rng = np.random.default_rng(E + n_members)
    T, n = 9, E * n_members
    # rewards of very different sizes: the order of the additions shows in the last bits
    reward = rng.standard_normal((T, n)) * 10.0 ** rng.integers(-6, 6, (T, n))
    reason = (rng.uniform(size=(T, n)) < 0.12).astype(np.uint8) * rng.integers(1, 4, (T, n)).astype(np.uint8)
    reason[0, 1] = 2                    # done at step 0: one reward, length 1
    reason[:, 2] = 0                    # never done: all T rewards
    reason[:, 5] = 0
    reward[3, 5] = np.nan               # a NaN reward while alive poisons that env and its member, nothing else
    reason[:2, 7] = 0
    reason[2, 7], reward[4, 7] = 1, np.nan      # ... and one after the episode has ended does not count
    got = P.population_fitness_ref(reward, reason, gamma, n_members)
    value, length, fitness, mean_len = _fitness_loops(reward.tolist(), reason.tolist(), gamma, n_members)
    assert got["env_value"].dtype == np.float64 and got["env_len"].dtype == np.int32
    assert _same(got["env_value"], value) and np.array_equal(got["env_len"], length)
    assert _same(got["fitness"], fitness) and _same(got["mean_len"], mean_len)
    assert got["env_len"][1] == 1 and got["env_value"][1] == reward[0, 1]
    assert got["env_len"][2] == T and np.isnan(got["env_value"][5]) and np.isnan(got["fitness"][0])
    assert got["env_len"][7] == 3 and not np.isnan(got["env_value"][7])
    assert np.isfinite(got["fitness"][1:]).all() and np.isfinite(got["mean_len"]).all()
    for bad in ((reward[:, :-1], reason[:, :-1]), (reward, reason[:-1])):
        with pytest.raises(ValueError):
            P.population_fitness_ref(bad[0], bad[1], gamma, n_members)
    with pytest.raises(ValueError):
        P.population_fitness_ref(np.zeros((T, 96)), np.zeros((T, 96), np.uint8), gamma, 1)        # 96 envs per member: no multiple of 64


@pytest.mark.parametrize("E", [64, 192, 320, 1024])
def test_fitness_ref_carries_non_finite_values_and_signed_zeros_as_the_plain_loops_do(E):
    """What the non-finite runs of tests/test_gpu_population_shapes.py lean on: members that hold +inf alone, -inf alone, both, a
    NaN in a lane's first element, a NaN in a later one - and rewards of -0.0 in a lane's first env, whose value is +0.0 all the
    same: the rule starts from v = +0.0 and (+0.0) + (-0.0) is +0.0, so a restatement that started from the first product shows"""
    n_members, T, gamma = 6, 5, 0.97
    n = n_members * E
    rng = np.random.default_rng(E)
    reward = rng.standard_normal((T, n))
    reason = (rng.uniform(size=(T, n)) < 0.2).astype(np.uint8)
    reason[:2, :] = 0
    last = E - 1                                                # (with E = 64 every element is a lane's first)
    reward[1, 0 * E + 7] = np.inf
    reward[1, 1 * E + last] = -np.inf
    reward[0, 2 * E + 3], reward[1, 2 * E + last] = np.inf, -np.inf
    reward[1, 3 * E + 5] = np.nan                               # first trip of lane 5
    reward[0, 4 * E + last] = np.nan                            # the last trip of lane 63
    reward[:, 5 * E + 9] = -0.0
    reward[0, 5 * E + 10], reason[0, 5 * E + 10] = -0.0, 1
    got = P.population_fitness_ref(reward, reason, gamma, n_members)
    value, length, fitness, mean_len = _fitness_loops(reward.tolist(), reason.tolist(), gamma, n_members)
    assert _same(got["env_value"], value) and np.array_equal(got["env_len"], length)
    assert _same(got["fitness"], fitness) and _same(got["mean_len"], mean_len)
    f = got["fitness"]
    assert f[0] == np.inf and f[1] == -np.inf and np.isnan(f[2]) and np.isnan(f[3]) and np.isnan(f[4]) and np.isfinite(f[5])
    v = got["env_value"]
    assert v[5 * E + 9] == 0.0 and not np.signbit(v[5 * E + 9]) and v[5 * E + 10] == 0.0 and not np.signbit(v[5 * E + 10])
    assert np.isposinf(v).sum() == 2 and np.isneginf(v).sum() == 2 and np.isnan(v).sum() == 2


def _oracle_rollout(case, cfg):
    """the scenario of tests/_population_cases.py, greedy, on the oracle backend -> (reward, reason, action) histories"""
    n_members, E = C.SHAPES[case]
    spec, params = C.members(case)
    prop = C.staged(OraclePropagator, cfg, C.initial_conditions(n_members * E, C.IC_SEED[case]))
    return C.S.oracle_histories(prop, spec, params, C.T, C.K, E)


@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_the_population_scenario_is_not_vacuous_on_the_oracle(case):
    """The handle, the staggering, the constants and the policies of tests/test_gpu_population_shapes.py, greedy, on the oracle
    backend: every member has envs that end by LENGTH, envs that end by WHEELS, envs that never end, and values of both signs - and
    in cases a, b and c (more than one trip of the join's lane loop) the trips added in descending order or into two alternating
    accumulators give other bits than the definition's order in at least one member, in the fitness and in the sum of squares."""
    n_members, E = C.SHAPES[case]
    reward, reason, action = _oracle_rollout(case, C.config(FLAG_AUTO_RESET))
    w = C.assert_every_member_is_mixed(reward, reason, action, E)
    print(case, {k: (int(x.min()), int(x.max())) for k, x in w.items()})
    fit = P.population_fitness_ref(reward, reason, C.GAMMA, n_members)
    rows = P.population_outcomes_ref(reward, reason, action, C.GAMMA, E)
    assert len(set(action.ravel().tolist())) == 3 and np.isfinite(fit["env_value"]).all()
    by_member = fit["env_value"].reshape(n_members, E)          # of like magnitude: within a factor of four of each other
    ratio = by_member.max(axis=1) / -by_member.min(axis=1)
    assert (by_member.min(axis=1) < 0).all() and (ratio > 0.25).all() and (ratio < 4.0).all(), ratio
    if E > 64:
        counts = C.assert_order_is_visible(fit["env_value"], E, fit["fitness"], rows[:, 8])
        print(case, counts)


@pytest.mark.parametrize("reward_mult", [C.REWARD_MULT, C.INF])
def test_the_non_finite_scenario_puts_a_nan_in_a_first_and_in_a_later_trip_on_the_oracle(reward_mult):
    n_members, E = C.SHAPES["n"]
    reward, reason, action = _oracle_rollout("n", C.config(FLAG_AUTO_RESET, reward_mult, C.INF))
    v = P.population_fitness_ref(reward, reason, C.GAMMA, n_members)["env_value"].reshape(n_members, E)
    first_trip, later_trip = C.nan_positions(v, E)
    print("members with a NaN in a first / in a later trip:", first_trip, later_trip, "NaN", int(np.isnan(v).sum()), "-inf",
          int(np.isneginf(v).sum()), "+inf", int(np.isposinf(v).sum()), "finite", int(np.isfinite(v).sum()))
    if reward_mult == C.INF:
        assert first_trip >= 1 and later_trip >= 1 and not np.isnan(v).all(axis=1).any()
        assert np.isposinf(v).any() and np.isneginf(v).any() and np.isfinite(v).any()
        lanes = v.reshape(n_members, E // 64, 64)
        assert (np.isnan(lanes[:, 0]) & ~np.isnan(lanes[:, 1:]).all(axis=1)).any()
        assert (~np.isnan(lanes[:, 0]) & np.isnan(lanes[:, 1:]).any(axis=1)).any()
    else:
        assert not np.isnan(v).any() and (np.isneginf(v).any(axis=1) & np.isfinite(v).any(axis=1)).all()


def test_the_first_es_generation_has_its_champion_past_the_first_64_members_on_the_oracle():
    """case e of tests/test_gpu_population_shapes.py: generation 0 of run_generation with shared episodes, in sample mode, on the
    oracle backend - the member nobody beats is one a later trip of the 64 lanes of es_outcome_kernel holds, and by a margin no
    last bit decides"""
    n_members, E = C.SHAPES["e"]
    spec, theta0 = C.es_start()
    cfg = C.config(FLAG_AUTO_RESET, max_length=C.ES["max_length"])
    prop = C.es_handle(OraclePropagator, cfg, (n_members + C.ES["n_val"]) * E)
    fit = C.es_generation_on_the_oracle(prop, cfg, spec, theta0, 0)
    f = fit["fitness"][:n_members]
    order = np.argsort(-f, kind="stable")
    print("champion", int(order[0]), "fitness", f[order[0]], "runner-up", int(order[1]), f[order[1]])
    assert np.isfinite(f).all() and len(set(f.tolist())) == n_members
    assert order[0] >= 64 and f[order[0]] - f[order[1]] > 1e-3
    assert (fit["env_len"] <= C.ES["max_length"] + 1).all() and (fit["env_len"] >= 1).all()


def test_population_abi_without_a_device():
    lib = _lib.load()
    good = P.c_spec(P.check_spec((32, 32), "tanh", (32,)))
    bad = P.c_spec(P.check_spec((32, 32), "tanh", (32,)))
    bad.hidden[1] = 40
    params = np.zeros(100000, np.float32)
    out = ctypes.c_void_p()
    # the order of bsk_policy_create: the spec, then n_members, then the device
    assert lib.bsk_population_create(ctypes.byref(bad), 0, params.ctypes.data, 0, ctypes.byref(out)) == -1 and not out.value
    assert lib.bsk_last_error().startswith(b"bsk_policy_spec")
    good.struct_size = 8
    assert lib.bsk_population_create(ctypes.byref(good), 4, params.ctypes.data, 0, ctypes.byref(out)) == -5
    good.struct_size = ctypes.sizeof(good)
    assert lib.bsk_population_create(None, 4, params.ctypes.data, 0, ctypes.byref(out)) == -1
    for n_members in (0, -3, (1 << 22) + 1):
        assert lib.bsk_population_create(ctypes.byref(good), n_members, params.ctypes.data, 0, ctypes.byref(out)) == -1 and not out.value
        assert b"n_members" in lib.bsk_last_error()
    assert lib.bsk_population_create(ctypes.byref(good), 4, params.ctypes.data, 0, None) == -1
    # every entry point refuses a NULL population before it touches a device
    assert lib.bsk_population_set_params(None, params.ctypes.data) == -1
    assert lib.bsk_population_set_params_device(None, params.ctypes.data, 0, 1, None) == -1
    assert lib.bsk_population_get_member(None, 0, params.ctypes.data) == -1
    assert lib.bsk_population_set_rng(None, 1, 0) == -1 and lib.bsk_population_get_rng(None, None, None) == -1
    assert lib.bsk_population_act(None, None, 0, 64, 64, 0, 0, None, None, None, None, 0, None) == -1
    assert lib.bsk_population_rollout(None, None, 0, 1, 1, 1.0, *([None] * 10)) == -1
    lib.bsk_population_destroy(None)
    if not os.path.exists("/dev/kfd"):
        # legal arguments on a box without a GPU: no device, said loudly; NULL parameters are legal (all-zero members)
        assert lib.bsk_population_create(ctypes.byref(good), 4, params.ctypes.data, 0, ctypes.byref(out)) == -2 and not out.value
        assert lib.bsk_population_create(ctypes.byref(good), 4, None, 0, ctypes.byref(out)) == -2 and not out.value
        spec, block = seeded_policy((16,), "relu", None, seed=1)
        with pytest.raises(_lib.BskGpuUnavailable):
            P.PolicyPopulation(spec, np.stack([block, block]))
    # the Python argument rules come before the library
    spec, block = seeded_policy((16,), "relu", None, seed=1)
    for params_bad in (block, np.stack([block[:-1]] * 2), np.zeros((0, block.size), np.float32)):
        with pytest.raises(ValueError):
            P.PolicyPopulation(spec, params_bad)
    with pytest.raises(ValueError):
        P.PolicyPopulation(spec)


def test_member_blocks_round_trip_through_unpack_params():
    """P distinct members stacked as the rows of one array: every row is a block unpack_params reads back, layer for layer"""
    spec = P.check_spec((32, 16), "relu", (16,), "tanh")
    blocks = np.stack([seeded_policy((32, 16), "relu", (16,), seed=s, value_activation="tanh")[1] for s in range(4)])
    assert blocks.shape == (4, P.n_params(spec)) and len({b.tobytes() for b in blocks}) == 4
    for b in blocks:
        sc, sh, a, v = P.unpack_params(spec, b)
        assert np.array_equal(P.pack_params(spec, a, v, sc, sh), b)
        assert [w.shape for w, _ in a] == [(32, 5), (16, 32), (3, 16)] and [w.shape for w, _ in v] == [(16, 5), (1, 16)]


def test_centred_ranks_follow_the_beats_rule():
    nan = np.nan
    u = P.centred_ranks([1.0, nan, 3.0, 3.0, -np.inf, nan])
    # 3.0 (index 2) > 3.0 (index 3) > 1.0 > -inf > NaN (index 1) > NaN (index 5)
    assert np.array_equal(np.argsort(-u), [2, 3, 0, 4, 1, 5])
    assert u.max() == 0.5 and u.min() == -0.5 and abs(u.sum()) < 1e-15 and np.allclose(np.diff(np.sort(u)), 0.2)


def test_evolution_strategy_descends_a_quadratic():
    n = 30
    target = np.random.default_rng(0).normal(size=n)
    target[:10] = 0.0

    def run():
        es = P.EvolutionStrategy(np.zeros(n), population=16, sigma=0.1, lr=0.05, seed=1)
        first = es.ask()
        es.tell(-((first.astype(np.float64) - target) ** 2).sum(axis=1))
        for _ in range(199):
            members = es.ask()
            es.tell(-((members.astype(np.float64) - target) ** 2).sum(axis=1))
        return first, es.theta
    first, theta = run()
    assert first.dtype == np.float32 and first.shape == (16, n)
    # antithetic pairs around theta = 0, and the input scale / shift are never perturbed nor moved
    assert np.array_equal(first[0::2], -first[1::2]) and not first[:, :10].any() and first[:, 10:].all()
    assert not theta[:10].any()
    start = np.linalg.norm(target)
    assert np.linalg.norm(theta - target) < 0.1 * start
    again_first, again_theta = run()
    assert np.array_equal(first, again_first) and np.array_equal(theta, again_theta)          # seeded
    with pytest.raises(ValueError):
        P.EvolutionStrategy(np.zeros(n), population=5)
    es = P.EvolutionStrategy(np.zeros(n), population=4)
    with pytest.raises(RuntimeError):
        es.tell(np.zeros(4))
    es.ask()
    with pytest.raises(ValueError):
        es.tell(np.zeros(3))


def test_c_consumer_compiles_from_the_header_alone(tmp_path):
    src = os.path.join(ROOT, "tests", "c_abi", "c_abi_population.c")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", src,
                           "-o", str(tmp_path / "c_abi_population.o")])
    text = open(src).read()
    assert [line for line in text.splitlines() if line.startswith("#include") and '"' in line] == ['#include "bskgpu.h"']
