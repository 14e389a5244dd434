"""GPU: a step size per parameter behind the device evolution strategy, adapted by tell (bsk_es_set_sigma_adaptation; the *_sigma
kernels and es_rank_q_kernel in csrc/bsk_es.hip; contract in include/bskgpu.h), alone and in whole generations on shared episodes.

Every check is an EQUALITY of bits against policy.es_ask_sigma_ref / policy.es_tell_pgpe_ref (which tests/test_es_sigma_host.py
holds to an operation-by-operation restatement) or against code that already ships - no tolerance anywhere.  Shapes as in
tests/test_gpu_es_adam.py: P = 2 is one pair (63 empty lanes, and q_0 = 0: sigma cannot move), P = 130 has one lane with two terms
and a ranking thread past the members, P = 256 gives every lane two, P = 258 and 600 take es_rank_q_kernel over two and three
tiles and workgroups with the awkward values beyond the first (tests/_es_cases.py).
"""
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
BETA1, BETA2, EPS, WD = 0.9, 0.999, 1e-8, 1e-2
LR_SIGMA, MAX_CHANGE, SIGMA_MIN, SIGMA_MAX = 4.0, 0.2, 0.05, 0.2
RULE = (LR_SIGMA, MAX_CHANGE, SIGMA_MIN, SIGMA_MAX)
N_POOL = 41


def _members(pop):
    return np.stack([pop.member(m) for m in range(pop.n_members)])


def _fitness_cases(n_members, rng):
    """ties, a NaN and infinities in every shape (tests/test_gpu_es_adam.py)"""
    if n_members == 2:
        return [np.array(f) for f in ([1.0, 1.0], [np.nan, np.inf], [-np.inf, 0.25])]
    f = rng.normal(size=n_members)
    f[7] = f[3]                                # a tie
    f[10] = f[11] = np.nan                     # a NaN pair
    f[20], f[21], f[40], f[41 + 64] = np.inf, -np.inf, np.inf, np.nan
    return [f, np.roll(f, 1), np.zeros(n_members)] + beyond_one_tile(n_members, rng)


def _sigma0(n):
    return np.random.default_rng(77).uniform(0.06, 0.18, size=n)


def _make(spec, theta0, n_members, frozen, optimizer, seed=SEED, **kw):
    adam = dict(optimizer="adam", beta1=BETA1, beta2=BETA2, eps=EPS, weight_decay=WD) if optimizer == "adam" else {}
    adam.update(kw)
    return P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=0.1, lr=0.05, seed=seed, frozen=frozen, **adam)


PGPE = dict(sigma_adapt="pgpe", lr_sigma=LR_SIGMA, sigma_max_change=MAX_CHANGE, sigma_min=SIGMA_MIN, sigma_max=SIGMA_MAX)


def _branches(sv, fitness, frozen, generation):
    """From the restatement's sums: how many moving entries take each of the rule's four clamp branches in this tell"""
    _, r0, n_members = P._es_pair_sums(fitness, sv.size, SEED, generation, with_r=True)
    sg = sv[frozen:]
    d = ((LR_SIGMA / float(n_members)) * r0[frozen:]) * sg
    lim = MAX_CHANGE * sg
    up, down = d > lim, d < -lim
    n = sg + np.where(up, lim, np.where(down, -lim, d))
    return np.array([up.sum(), down.sum(), (n < SIGMA_MIN).sum(), (n > SIGMA_MAX).sum()])


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("frozen", [0, 10])
@pytest.mark.parametrize("n_members", [2, 130, 256, 258, 600])
def test_tell_is_the_definition(n_members, frozen, optimizer):
    import torch
    spec, theta0 = seeded_policy((16,), "relu", None, seed=9)
    n, lr = theta0.size, 0.05
    es = _make(spec, theta0, n_members, frozen, optimizer, **PGPE)
    assert _same(es.sigma_vector, np.full(n, 0.1)) and es.generation == 0
    sv0 = _sigma0(n)
    es.set_sigma(sv0)
    assert _same(es.sigma_vector, sv0)
    state = (theta0.astype(np.float64), sv0) + ((np.zeros(n), np.zeros(n), np.ones(2)) if optimizer == "adam" else ())
    generation, taken = 0, np.zeros(4, np.int64)
    for round_, f in enumerate(_fitness_cases(n_members, np.random.default_rng(n_members))):
        if round_ == 1:
            generation = LATE
            es.set_state(None, generation)
            assert _same(es.sigma_vector, state[1])            # set_state leaves the vector alone
        d_f = torch.from_numpy(f).cuda()
        torch.cuda.synchronize()
        c0 = BatchedPropagator.debug_counters()
        es.tell(d_f)
        assert BatchedPropagator.debug_counters() == c0            # three launches: no copy, no synchronisation
        taken += _branches(state[1], f, frozen, generation)
        state = P.es_tell_pgpe_ref(state[0], state[1], f, lr, frozen, SEED, generation, *RULE,
                                   adam=None if optimizer == "sgd" else tuple(state[2:]) + (BETA1, BETA2, EPS, WD))
        got = (es.theta, es.sigma_vector) + (es.moments if optimizer == "adam" else ())
        for g, w, name in zip(got, state, ("theta", "sigma", "m", "v", "beta_pow")):
            assert _same(g, w), (round_, name)
        assert _same(got[0][:frozen], theta0[:frozen].astype(np.float64)) and _same(got[1][:frozen], sv0[:frozen])
        assert np.isfinite(got[0]).all()
        if n_members == 2:
            assert _same(got[1], sv0)                              # q_0 = 0: the bits never change
        generation += 1
        assert es.generation == generation
    if n_members > 2:
        # the checks above went through every branch of the rule, and not only through its clamps
        assert (taken >= 1).all(), taken
        inside = (state[1][frozen:] > SIGMA_MIN) & (state[1][frozen:] < SIGMA_MAX)
        assert 2 * inside.sum() >= n - frozen, inside.sum()
    with pytest.raises(ValueError):
        es.set_sigma(np.full(n + 1, 0.1))
    es.close()


@pytest.mark.parametrize("frozen", [0, 10])
@pytest.mark.parametrize("n_members", [2, 130, 256, 258, 600])
def test_ask_is_the_definition(n_members, frozen):
    spec, theta0 = seeded_policy((16,), "relu", None, seed=9)
    n = theta0.size
    es = _make(spec, theta0, n_members, frozen, "sgd", **PGPE)
    pop = P.PolicyPopulation(spec, n_members=n_members)
    sv = _sigma0(n)
    es.set_sigma(sv)
    seen = []
    for generation in (0, LATE):
        es.set_state(None, generation)
        es.ask(pop)
        got = _members(pop)
        assert _same(got, P.es_ask_sigma_ref(theta0, sv, frozen, n_members, SEED, generation)), generation
        assert _same(got[:, :frozen], np.broadcast_to(theta0[:frozen], (n_members, frozen))) and not _same(got[0], got[1])
        assert es.generation == generation and _same(es.sigma_vector, sv)          # ask leaves both alone
        seen.append(got)
    assert not _same(seen[0], seen[1]) and not _same(seen[0], P.es_ask_ref(theta0, 0.1, frozen, n_members, SEED, 0))
    es.close()
    pop.close()


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("n_members", [2, 130, 256, 258, 600])
def test_a_uniform_vector_with_lr_sigma_zero_is_the_optimiser_that_never_selected_the_mode(n_members, optimizer):
    import torch
    frozen = 10
    spec, theta0 = seeded_policy((16,), "relu", None, seed=9)
    n = theta0.size
    plain = _make(spec, theta0, n_members, frozen, optimizer)
    es = _make(spec, theta0, n_members, frozen, optimizer, sigma_adapt="pgpe", lr_sigma=0.0, sigma_max_change=MAX_CHANGE,
               sigma_min=SIGMA_MIN, sigma_max=SIGMA_MAX)
    pops = [P.PolicyPopulation(spec, n_members=n_members) for _ in range(2)]
    for round_, f in enumerate(_fitness_cases(n_members, np.random.default_rng(n_members))):
        for opt, pop in zip((plain, es), pops):
            opt.ask(pop)
        assert _same(_members(pops[0]), _members(pops[1])), round_
        d_f = torch.from_numpy(f).cuda()
        plain.tell(d_f)
        es.tell(d_f)
        assert _same(es.theta, plain.theta) and es.generation == plain.generation == round_ + 1
        assert _same(es.sigma_vector, np.full(n, 0.1))
        if optimizer == "adam":
            for got, want in zip(es.moments, plain.moments):
                assert _same(got, want)
    # FIXED again: the creation sigma's tell, whatever the vector holds; theta, the generation and the moments stayed
    es.set_sigma(_sigma0(n))
    theta, generation = es.theta, es.generation
    moments = es.moments if optimizer == "adam" else None
    es.set_sigma_adaptation(None)
    assert _same(es.theta, theta) and es.generation == generation
    with pytest.raises(_lib.BskError):
        es.sigma_vector
    f = np.random.default_rng(2).normal(size=n_members)
    es.ask(pops[0])
    assert _same(_members(pops[0]), P.es_ask_ref(theta, 0.1, frozen, n_members, SEED, generation))
    es.tell(torch.from_numpy(f).cuda())
    if optimizer == "sgd":
        assert _same(es.theta, P.es_tell_ref(theta, f, 0.1, 0.05, frozen, SEED, generation))
    else:
        want = P.es_tell_adam_ref(theta, *moments, f, 0.1, 0.05, frozen, SEED, generation, BETA1, BETA2, EPS, WD)
        for g, w in zip((es.theta,) + es.moments, want):
            assert _same(g, w)
    # selected again, the vector is the creation sigma's; set_optimizer leaves it alone
    es.set_sigma_adaptation("pgpe", *RULE)
    assert _same(es.sigma_vector, np.full(n, 0.1))
    es.set_sigma(_sigma0(n))
    es.set_optimizer("adam", BETA1, BETA2, EPS, WD)
    es.set_optimizer("sgd")
    assert _same(es.sigma_vector, _sigma0(n))
    for x in [plain, es] + pops:
        x.close()


def _propagator(n, ic, pool, stream=None):
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    cfg.max_length = 6
    p = BatchedPropagator(cfg, n, stream=stream)
    p.set_ic_pool(pool)
    p.reset(ic)
    p.step(np.zeros(n, np.int32), 1)
    return p


def test_generations_carry_the_vector_forward_on_the_device_and_replay_from_a_hip_graph():
    import torch
    n_members, E, T, k, gamma = 4, 64, 8, 1, 0.99
    n = n_members * E
    spec, theta0 = seeded_policy((16,), "tanh", None, seed=5)
    lr, frozen, seed = 0.05, 10, 3
    np_ = theta0.size
    ic = sample_ic_batch(n, 4, seed=29)
    pool = sample_ic_batch(N_POOL, 4, seed=15)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        # the reference: three generations composed on the host from pieces that already ship and the two restatements; a host
        # reset from the initial conditions shared_slot_ref names stands in for the device reset
        prop = _propagator(n, ic, pool, side.cuda_stream)
        pop = P.PolicyPopulation(spec, n_members=n_members)
        d_fit = torch.full((n_members,), -7.0, dtype=torch.float64, device="cuda")
        state, want = (theta0.astype(np.float64), np.full(np_, 0.1), np.zeros(np_), np.zeros(np_), np.ones(2)), []
        for g in range(3):
            pop.set_params(P.es_ask_sigma_ref(state[0], state[1], frozen, n_members, seed, g))
            prop.reset(pool[:, P.shared_slot_ref(n, E, g, N_POOL)])
            pop.rollout_device(prop, T, k, "greedy", gamma, d_fitness=d_fit.data_ptr())
            prop.sync()
            fitness = d_fit.cpu().numpy()
            state = P.es_tell_pgpe_ref(state[0], state[1], fitness, lr, frozen, seed, g, *RULE, adam=tuple(state[2:]) + (BETA1, BETA2, EPS, WD))
            want.append((state[0], fitness, state[1]))
        assert np.isfinite(want[2][1]).all() and not _same(want[0][1], want[1][1]) and not _same(want[0][0], want[2][0])
        # the vector differs from generation to generation: what runs below has to carry it forward
        assert not _same(want[0][2], np.full(np_, 0.1)) and not _same(want[0][2], want[1][2]) and not _same(want[1][2], want[2][2])
        prop.close()
        pop.close()

        def make():
            prop = _propagator(n, ic, pool, side.cuda_stream)
            pop = P.PolicyPopulation(spec, n_members=n_members)
            return prop, pop, _make(spec, theta0, n_members, frozen, "adam", seed=seed, **PGPE)

        def result(es):
            theta = es.theta                                # (synchronises the device)
            return theta, _download(es.fitness_buffer().ptr, np.float64, n_members), es.sigma_vector

        prop, pop, es = make()
        for g in range(3):
            c0 = BatchedPropagator.debug_counters()
            es.run_generation(prop, pop, T, k, "greedy", gamma, shared_episodes=True)
            if g:
                assert BatchedPropagator.debug_counters() == c0      # no copy, no synchronisation
            for got, w, name in zip(result(es), want[g], ("theta", "fitness", "sigma")):
                assert _same(got, w), (g, name)
            assert es.generation == g + 1
        for got, w in zip(es.moments, state[2:]):
            assert _same(got, w)
        for x in (prop, pop, es):
            x.close()

        # captured once behind a warming call, replayed twice: generations two and three of the run above - sigma_vec is device
        # state, so each replay asks with the vector the tell before it left
        prop, pop, es = make()
        es.run_generation(prop, pop, T, k, "greedy", gamma, shared_episodes=True)
        prop.sync()
        assert _same(result(es)[2], want[0][2])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            es.run_generation(prop, pop, T, k, "greedy", gamma, shared_episodes=True)
        for g in (1, 2):
            c0 = BatchedPropagator.debug_counters()
            graph.replay()
            torch.cuda.synchronize()
            assert BatchedPropagator.debug_counters() == c0
            for got, w, name in zip(result(es), want[g], ("theta", "fitness", "sigma")):
                assert _same(got, w), (g, name)
            assert es.generation == g + 1
        for got, w in zip(es.moments, state[2:]):
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
    fixed = P.DeviceEvolutionStrategy(spec, theta0, n_members, seed=2)
    pgpe = P.DeviceEvolutionStrategy(spec, theta0, n_members, seed=2, optimizer="adam", sigma_adapt="pgpe", lr_sigma=0.5,
                                     sigma_max_change=0.25, sigma_min=0.02, sigma_max=0.5)
    sv0, m0, v0 = np.random.default_rng(3).uniform(0.05, 0.3, size=n), np.full(n, 0.25), np.full(n, 0.5)
    pgpe.set_sigma(sv0)
    pgpe.set_moments(m0, v0, [0.75, 0.875])
    d_fit = torch.tensor([0.5, -1.0, 2.0, 0.0], dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    buf = np.zeros(n)
    good = (0.1, 0.2, 0.01, 1.0)
    bad = ([(2,) + good, (-1,) + good] + [(1, x, 0.2, 0.01, 1.0) for x in (-1e-3, nan, inf, -inf)] +
           [(1, 0.1, x, 0.01, 1.0) for x in (0.0, 1.0, -0.2, 1.5, nan, inf)] + [(1, 0.1, 0.2, x, 1.0) for x in (0.0, -0.01, nan, inf, -inf)] +
           [(1, 0.1, 0.2, 0.01, x) for x in (0.005, nan, inf, -inf)] +
           [(1, 0.1, 0.2, 0.2, 1.0), (1, 0.1, 0.2, 0.01, 0.05)])              # the creation sigma, 0.1, outside the bounds
    c0 = BatchedPropagator.debug_counters()
    for handle in (fixed._handle(), pgpe._handle()):
        for args in bad:
            assert lib.bsk_es_set_sigma_adaptation(handle, *args) == -1, args
            assert b"bsk_es_set_sigma_adaptation" in lib.bsk_last_error()
    assert lib.bsk_es_set_sigma_adaptation(None, 1, *good) == -1
    # no vector while the kind is FIXED
    assert lib.bsk_es_get_sigma(fixed._handle(), buf.ctypes.data) == -1 and b"FIXED" in lib.bsk_last_error()
    assert lib.bsk_es_set_sigma(fixed._handle(), buf.ctypes.data) == -1 and b"FIXED" in lib.bsk_last_error()
    assert lib.bsk_es_get_sigma(None, buf.ctypes.data) == -1 and lib.bsk_es_set_sigma(None, buf.ctypes.data) == -1
    assert lib.bsk_es_get_sigma(pgpe._handle(), None) == -1 and lib.bsk_es_set_sigma(pgpe._handle(), None) == -1
    # an entry that is not finite and positive: nothing is written
    for x in (0.0, -0.1, nan, inf):
        wrong = sv0.copy()
        wrong[n - 1] = x
        assert lib.bsk_es_set_sigma(pgpe._handle(), wrong.ctypes.data) == -1 and b"bsk_es_set_sigma" in lib.bsk_last_error()
    assert BatchedPropagator.debug_counters() == c0
    # FIXED ignores the other arguments
    assert lib.bsk_es_set_sigma_adaptation(fixed._handle(), 0, nan, 7.0, -1.0, -inf) == 0
    # nothing moved: the fixed optimiser still takes the plain step, the other kept its vector, its moments and its constants
    assert _same(fixed.theta, theta0.astype(np.float64)) and fixed.generation == 0
    assert _same(pgpe.sigma_vector, sv0) and _same(pgpe.theta, theta0.astype(np.float64)) and pgpe.generation == 0
    got = pgpe.moments
    assert _same(got[0], m0) and _same(got[1], v0) and _same(got[2], np.array([0.75, 0.875]))
    f = d_fit.cpu().numpy()
    fixed.tell(d_fit)
    pgpe.tell(d_fit)
    assert _same(fixed.theta, P.es_tell_ref(theta0, f, 0.1, 0.05, 10, 2, 0))
    want = P.es_tell_pgpe_ref(theta0, sv0, f, 0.05, 10, 2, 0, 0.5, 0.25, 0.02, 0.5, adam=(m0, v0, [0.75, 0.875], 0.9, 0.999, 1e-8, 0.0))
    for g, w in zip((pgpe.theta, pgpe.sigma_vector) + pgpe.moments, want):
        assert _same(g, w)
    assert not _same(want[1], sv0)
    fixed.close()
    pgpe.close()
    with pytest.raises(RuntimeError):
        pgpe.sigma_vector


def test_c_consumer_prints_the_python_bindings_sigma(tmp_path):
    """tests/c_abi/c_abi_es_sigma.c: bsk_es_set_sigma_adaptation / bsk_es_set_sigma / bsk_es_get_sigma from plain C99, two
    generations on a 128-env handle; its hex-float printout equals the Python binding's"""
    exe = build_c_consumer(tmp_path, "c_abi_es_sigma")
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
    es = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=0.1, lr=0.05, seed=SEED, frozen=10, sigma_adapt="pgpe", lr_sigma=0.5,
                                   sigma_max_change=0.2, sigma_min=0.01, sigma_max=1.0)
    np_ = P.n_params(spec)
    sv0 = np.array([0.05 + 0.001 * float(j % 100) for j in range(np_)])
    es.set_sigma(sv0)
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
    theta, sigma = es.theta, es.sigma_vector
    want += theta.tolist() + sigma.tolist() + [float(es.generation)]
    assert len(got) == len(want) == 2 * n_members + 2 * np_ + 1
    assert [float.fromhex(x) for x in got] == want
    assert want[-1] == 2.0 and want[:n_members] != want[n_members:2 * n_members]
    # one pair: the vector the C program set is the vector it printed, and theta moved by it
    assert _same(sigma, sv0) and not _same(theta[10:], theta0[10:].astype(np.float64))
    d_fit.free()
    for x in (es, pop, prop):
        x.close()
