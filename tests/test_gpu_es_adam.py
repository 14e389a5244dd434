"""GPU: Adam with an L2 penalty behind the device evolution strategy's tell (bsk_es_set_optimizer; es_tell_adam_kernel in
csrc/bsk_es.hip; contract in include/bskgpu.h), alone and in whole generations on shared episodes.

Every check is an EQUALITY of bits against policy.es_tell_adam_ref (which tests/test_es_adam_host.py holds to an operation-by-
operation restatement) or against code that already ships - no tolerance anywhere.  Shapes as in tests/test_gpu_es.py: P = 2 is one
pair (63 empty lanes), P = 130 has one lane with two terms and a ranking thread past the members, P = 256 gives every lane two,
P = 258 and 600 rank over two and three tiles and workgroups with the awkward values beyond the first (tests/_es_cases.py).
"""
import ctypes
import subprocess

import numpy as np
import pytest

from _device_bits import build_c_consumer, download as _download, same as _same
from _es_cases import beyond_one_tile
from _policy_bounds import seeded_policy
from basilisk_env_amd import _hip, _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch

pytestmark = pytest.mark.gpu

SEED, LATE = 2 ** 33 + 5, 2 ** 32 + 3
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
N_POOL = 41


def _fitness_cases(n_members, rng):
    """ties, a NaN and infinities in every shape"""
    if n_members == 2:
        return [np.array(f) for f in ([1.0, 1.0], [np.nan, np.inf], [-np.inf, 0.25])]
    f = rng.normal(size=n_members)
    f[7] = f[3]                                # a tie
    f[10] = f[11] = np.nan                     # a NaN pair
    f[20], f[21], f[40], f[41 + 64] = np.inf, -np.inf, np.inf, np.nan
    return [f, np.roll(f, 1), np.zeros(n_members)] + beyond_one_tile(n_members, rng)


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
@pytest.mark.parametrize("frozen", [0, 10])
@pytest.mark.parametrize("n_members", [2, 130, 256, 258, 600])
def test_adam_tell_is_the_definition(n_members, frozen, weight_decay):
    import torch
    spec, theta0 = seeded_policy((16,), "relu", None, seed=9)
    n, sigma, lr = theta0.size, 0.1, 0.05
    es = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=sigma, lr=lr, seed=SEED, frozen=frozen, optimizer="adam", beta1=BETA1,
                                   beta2=BETA2, eps=EPS, weight_decay=weight_decay)
    m, v, beta_pow = es.moments
    assert not m.any() and not v.any() and _same(beta_pow, np.ones(2)) and es.generation == 0
    state = (theta0.astype(np.float64), m, v, beta_pow)
    generation = 0
    for round_, f in enumerate(_fitness_cases(n_members, np.random.default_rng(n_members))):
        if round_ == 1:
            generation = LATE
            es.set_state(None, generation)
        d_f = torch.from_numpy(f).cuda()
        torch.cuda.synchronize()
        c0 = BatchedPropagator.debug_counters()
        es.tell(d_f)
        assert BatchedPropagator.debug_counters() == c0            # three launches: no copy, no synchronisation
        state = P.es_tell_adam_ref(*state, f, sigma, lr, frozen, SEED, generation, BETA1, BETA2, EPS, weight_decay)
        got = (es.theta,) + es.moments
        for g, w, name in zip(got, state, ("theta", "m", "v", "beta_pow")):
            assert _same(g, w), (round_, name)
        assert _same(got[0][:frozen], theta0[:frozen].astype(np.float64)) and not got[1][:frozen].any() and not got[2][:frozen].any()
        assert np.isfinite(got[0]).all()
        generation += 1
        assert es.generation == generation
    assert state[1][frozen:].any() and (state[2][frozen:] > 0.0).all()

    # the moments travel to the device and back; None keeps
    rng = np.random.default_rng(1)
    m2, v2, bp2 = rng.normal(size=n), rng.uniform(size=n), np.array([0.5, 0.25])
    es.set_moments(m2, None, bp2)
    got = es.moments
    assert _same(got[0], m2) and _same(got[1], state[2]) and _same(got[2], bp2)
    es.set_moments(v=v2)
    assert _same(es.moments[1], v2) and _same(es.moments[0], m2)
    f = np.random.default_rng(2).normal(size=n_members)
    theta = es.theta
    es.tell(torch.from_numpy(f).cuda())
    want = P.es_tell_adam_ref(theta, m2, v2, bp2, f, sigma, lr, frozen, SEED, generation, BETA1, BETA2, EPS, weight_decay)
    for g, w in zip((es.theta,) + es.moments, want):
        assert _same(g, w)
    with pytest.raises(ValueError):
        es.set_moments(m=np.zeros(n + 1))

    # SGD again is the plain step; Adam selected again starts from zero moments, theta and the generation stay
    theta, generation = es.theta, es.generation
    es.set_optimizer("sgd")
    assert _same(es.theta, theta) and es.generation == generation
    with pytest.raises(_lib.BskError):
        es.moments
    es.tell(torch.from_numpy(f).cuda())
    theta = P.es_tell_ref(theta, f, sigma, lr, frozen, SEED, generation)
    assert _same(es.theta, theta) and es.generation == generation + 1
    es.set_optimizer("adam", BETA1, BETA2, EPS, weight_decay)
    m, v, beta_pow = es.moments
    assert not m.any() and not v.any() and _same(beta_pow, np.ones(2)) and _same(es.theta, theta) and es.generation == generation + 1
    es.close()


def _propagator(n, ic, pool, stream=None):
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    cfg.max_length = 6
    p = BatchedPropagator(cfg, n, stream=stream)
    p.set_ic_pool(pool)
    p.reset(ic)
    p.step(np.zeros(n, np.int32), 1)
    return p


def test_adam_generations_on_shared_episodes_run_on_the_device_and_replay_from_a_hip_graph():
    import torch
    n_members, E, T, k, gamma = 4, 64, 8, 1, 0.99
    n = n_members * E
    spec, theta0 = seeded_policy((16,), "tanh", None, seed=5)
    sigma, lr, frozen, seed, wd = 0.1, 0.05, 10, 3, 1e-2
    ic = sample_ic_batch(n, 4, seed=29)
    pool = sample_ic_batch(N_POOL, 4, seed=15)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        # the reference: three generations composed on the host from pieces that already ship and the two restatements; a host
        # reset from the initial conditions shared_slot_ref names stands in for the device reset
        prop = _propagator(n, ic, pool, side.cuda_stream)
        pop = P.PolicyPopulation(spec, n_members=n_members)
        d_fit = torch.full((n_members,), -7.0, dtype=torch.float64, device="cuda")
        state, want, slots = (theta0.astype(np.float64), np.zeros(theta0.size), np.zeros(theta0.size), np.ones(2)), [], []
        for g in range(3):
            pop.set_params(P.es_ask_ref(state[0], sigma, frozen, n_members, seed, g))
            slots.append(P.shared_slot_ref(n, E, g, N_POOL))
            prop.reset(pool[:, slots[-1]])
            pop.rollout_device(prop, T, k, "greedy", gamma, d_fitness=d_fit.data_ptr())
            prop.sync()
            fitness = d_fit.cpu().numpy()
            state = P.es_tell_adam_ref(*state, fitness, sigma, lr, frozen, seed, g, BETA1, BETA2, EPS, wd)
            want.append((state[0], fitness))
        # successive generations start from different slots and are scored differently
        assert not np.array_equal(slots[0], slots[1]) and not np.array_equal(slots[1], slots[2])
        assert np.isfinite(want[2][1]).all() and not _same(want[0][1], want[1][1]) and not _same(want[0][0], want[2][0])
        prop.close()
        pop.close()

        def make():
            prop = _propagator(n, ic, pool, side.cuda_stream)
            pop = P.PolicyPopulation(spec, n_members=n_members)
            es = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=sigma, lr=lr, seed=seed, frozen=frozen, optimizer="adam",
                                           beta1=BETA1, beta2=BETA2, eps=EPS, weight_decay=wd)
            return prop, pop, es

        def result(es):
            theta = es.theta                                # (synchronises the device)
            return theta, _download(es.fitness_buffer().ptr, np.float64, n_members)

        prop, pop, es = make()
        for g in range(3):
            c0 = BatchedPropagator.debug_counters()
            es.run_generation(prop, pop, T, k, "greedy", gamma, shared_episodes=True)
            if g:
                assert BatchedPropagator.debug_counters() == c0      # no copy, no synchronisation
            got = result(es)
            assert _same(got[0], want[g][0]) and _same(got[1], want[g][1]), g
            assert es.generation == g + 1
        for got, w in zip(es.moments, state[1:]):
            assert _same(got, w)
        for x in (prop, pop, es):
            x.close()

        # captured once behind a warming call, replayed twice: generations two and three of the run above - the epoch is a device
        # word, so the replays draw the slots of THEIR generation
        prop, pop, es = make()
        es.run_generation(prop, pop, T, k, "greedy", gamma, shared_episodes=True)
        prop.sync()
        assert _same(result(es)[0], want[0][0])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            es.run_generation(prop, pop, T, k, "greedy", gamma, shared_episodes=True)
        for g in (1, 2):
            c0 = BatchedPropagator.debug_counters()
            graph.replay()
            torch.cuda.synchronize()
            assert BatchedPropagator.debug_counters() == c0
            got = result(es)
            assert _same(got[0], want[g][0]) and _same(got[1], want[g][1]), g
            assert es.generation == g + 1
        for got, w in zip(es.moments, state[1:]):
            assert _same(got, w)
        for x in (prop, pop, es):
            x.close()


def test_refusals_come_before_any_launch():
    import torch
    lib = _lib.load()
    n_members = 4
    spec, theta0 = seeded_policy((16,), "relu", None, seed=21)
    n = theta0.size
    nan, inf = float("nan"), float("inf")
    es = P.DeviceEvolutionStrategy(spec, theta0, n_members, seed=2)
    adam = P.DeviceEvolutionStrategy(spec, theta0, n_members, seed=2, optimizer="adam")
    m0, v0 = np.full(n, 0.25), np.full(n, 0.5)
    adam.set_moments(m0, v0, [0.75, 0.875])
    d_fit = torch.tensor([0.5, -1.0, 2.0, 0.0], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    buf = np.zeros(n)
    p = ctypes.c_void_p()
    c0 = BatchedPropagator.debug_counters()
    bad = ([(2,) + (BETA1, BETA2, EPS, 0.0), (-1,) + (BETA1, BETA2, EPS, 0.0)] +
           [(1, b, BETA2, EPS, 0.0) for b in (-0.1, 1.0, 1.5, nan, inf)] + [(1, BETA1, b, EPS, 0.0) for b in (-0.1, 1.0, nan, -inf)] +
           [(1, BETA1, BETA2, e, 0.0) for e in (0.0, -1e-8, nan, inf)] + [(1, BETA1, BETA2, EPS, d) for d in (-1e-3, nan, inf)])
    for handle in (es._handle(), adam._handle()):
        for args in bad:
            assert lib.bsk_es_set_optimizer(handle, *args) == -1, args
            assert b"bsk_es_set_optimizer" in lib.bsk_last_error()
    assert lib.bsk_es_set_optimizer(None, 1, BETA1, BETA2, EPS, 0.0) == -1
    # no moments while the optimiser is SGD
    assert lib.bsk_es_get_moments(es._handle(), buf.ctypes.data, None, None) == -1 and b"SGD" in lib.bsk_last_error()
    assert lib.bsk_es_set_moments(es._handle(), buf.ctypes.data, None, None) == -1 and b"SGD" in lib.bsk_last_error()
    assert lib.bsk_es_get_moments(None, None, None, None) == -1 and lib.bsk_es_set_moments(None, None, None, None) == -1
    assert lib.bsk_es_generation_device(None, ctypes.byref(p)) == -1 and lib.bsk_es_generation_device(es._handle(), None) == -1
    assert BatchedPropagator.debug_counters() == c0
    # SGD ignores the other arguments
    assert lib.bsk_es_set_optimizer(es._handle(), 0, nan, 7.0, -1.0, -inf) == 0
    # nothing moved: the SGD optimiser still takes the plain step, the Adam one kept its moments and its constants
    assert _same(es.theta, theta0.astype(np.float64)) and es.generation == 0
    got = adam.moments
    assert _same(got[0], m0) and _same(got[1], v0) and _same(got[2], np.array([0.75, 0.875])) and adam.generation == 0
    f = d_fit.cpu().numpy()
    es.tell(d_fit)
    adam.tell(d_fit)
    assert _same(es.theta, P.es_tell_ref(theta0, f, 0.1, 0.05, 10, 2, 0))
    want = P.es_tell_adam_ref(theta0, m0, v0, [0.75, 0.875], f, 0.1, 0.05, 10, 2, 0, 0.9, 0.999, 1e-8, 0.0)
    for g, w in zip((adam.theta,) + adam.moments, want):
        assert _same(g, w)
    # the generation word is the optimiser's counter
    word = adam.generation_ptr()
    assert word and _download(word, np.uint64, 1)[0] == 1 == adam.generation
    adam.set_state(None, LATE)
    assert _download(word, np.uint64, 1)[0] == LATE and adam.generation_ptr() == word
    es.close()
    adam.close()
    with pytest.raises(RuntimeError):
        adam.generation_ptr()


def test_c_consumer_prints_the_python_bindings_adam_state(tmp_path):
    """tests/c_abi/c_abi_es_adam.c: bsk_es_set_optimizer / bsk_es_generation_device / bsk_reset_from_pool_shared / bsk_es_get_moments
    from plain C99, two generations on a 128-env handle; its hex-float printout equals the Python binding's"""
    exe = build_c_consumer(tmp_path, "c_abi_es_adam")
    n_members, n = 2, 128                                   # (a member drives a multiple of 64 envs)
    E = n // n_members
    pool = sample_ic_batch(N_POOL, 4, seed=53)
    spec, theta0 = seeded_policy((16,), "relu", None, seed=97)
    pool.tofile(tmp_path / "pool.bin")
    theta0.tofile(tmp_path / "theta.bin")
    got = subprocess.check_output([str(exe), str(tmp_path / "pool.bin"), str(N_POOL), str(tmp_path / "theta.bin"), str(n_members)]).decode().split()
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    prop = BatchedPropagator(cfg, n)
    prop.set_ic_pool(pool)
    es = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=0.1, lr=0.05, seed=SEED, frozen=10, optimizer="adam", beta1=0.9,
                                   beta2=0.999, eps=1e-8, weight_decay=1e-2)
    pop = P.PolicyPopulation(spec, n_members=n_members)
    d_fit = _hip.DeviceBuffer(8 * n_members, 0)
    want = []
    for _ in range(2):
        prop.reset_from_pool_shared(E, es.generation_ptr())
        es.ask(pop, prop.stream_ptr())
        pop.rollout_device(prop, 6, 5, "greedy", 0.97, d_fitness=d_fit.ptr)
        es.tell(d_fit.ptr, prop.stream_ptr())
        prop.sync()
        want += _download(d_fit.ptr, np.float64, n_members).tolist()
    m, v, beta_pow = es.moments
    want += es.theta.tolist() + m.tolist() + v.tolist() + beta_pow.tolist() + [float(es.generation)]
    np_ = P.n_params(spec)
    assert len(got) == len(want) == 2 * n_members + 3 * np_ + 2 + 1
    assert [float.fromhex(x) for x in got] == want
    assert want[-1] == 2.0 and want[:n_members] != want[n_members:2 * n_members] and any(m) and any(v)
    assert _same(beta_pow, np.array([0.9 * 0.9, 0.999 * 0.999]))
    d_fit.free()
    for x in (es, pop, prop):
        x.close()
