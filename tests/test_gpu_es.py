"""GPU: the evolution strategy on the device (bsk_es_*; kernels in csrc/bsk_es.hip; contract in include/bskgpu.h).

Every check is an EQUALITY of bits against the numpy restatement (policy.es_ask_ref / es_tell_ref, which tests/test_es_host.py
holds to mpmath, to the plain matrix product and to EvolutionStrategy) or against code that already ships - no tolerance anywhere.
Shapes: P = 2 is one pair (63 empty lanes in tell's sum), P = 130 is 65 pairs (one lane with two terms, and a ranking with one
thread past the members), P = 256 gives every lane two terms; P = 258 and 600 take the ranking past one tile of 256 values and one
workgroup (258: a second workgroup and a second tile of exactly one pair; 600: three tiles, a partial third workgroup, and 300
pairs, so lanes with five and with four terms), with ties, NaNs and infinities on the far side of the boundaries
(tests/_es_cases.py); the tanh spec has a value network, whose fan-outs 3 and 1 are padded in the device layout; generation
2^32 + 3 and seed 2^33 + 5 catch a dropped high word.

The far tail of the inverse normal CDF (r > 5: p < e^-25, 2.8e-11 per draw) is reached by choosing the key: the seeds of
tests/golden/es_tail_seeds.json (found by tools/es_tail_seeds.c; tests/test_es_host.py holds the restatement there to mpmath) make
the first draw of one parameter a |z| of about 6.8.
"""
import ctypes
import subprocess

import numpy as np
import pytest

from _device_bits import build_c_consumer, download as _download, same as _same
from _es_cases import beyond_one_tile, tail_rows
from _policy_bounds import observation_like, seeded_policy
from basilisk_env_amd import _hip, _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch

pytestmark = pytest.mark.gpu

SEED, LATE = 2 ** 33 + 5, 2 ** 32 + 3
SPECS = {"relu16": ((16,), "relu", None), "tanh16x32v16": ((16, 32), "tanh", (16,))}


def _members(pop):
    return np.stack([pop.member(m) for m in range(pop.n_members)])


@pytest.mark.parametrize("frozen", [10, 0])
@pytest.mark.parametrize("which", sorted(SPECS))
@pytest.mark.parametrize("n_members", [2, 130, 258, 600])
def test_ask_writes_the_members_of_the_definition(n_members, which, frozen):
    import torch
    hidden, activation, value_hidden = SPECS[which]
    spec, theta = seeded_policy(hidden, activation, value_hidden, seed=7)
    sigma, n = 0.1, 64 * n_members
    es = P.DeviceEvolutionStrategy(spec, theta, n_members, sigma=sigma, lr=0.05, seed=SEED, frozen=frozen)
    pop = P.PolicyPopulation(spec, n_members=n_members)
    other = P.PolicyPopulation(spec, n_members=n_members)
    assert _same(es.theta, theta.astype(np.float64)) and es.generation == 0
    obs = torch.from_numpy(observation_like(n, seed=n_members)).cuda()
    want_out = ("logits", "value") if value_hidden is not None else ("logits",)
    seen = []
    for generation in (0, LATE):
        if generation:
            es.set_state(None, generation)
        assert es.generation == generation
        es.ask(pop)
        want = P.es_ask_ref(theta, sigma, frozen, n_members, SEED, generation)
        got = _members(pop)
        assert _same(got, want), generation
        assert _same(got[:, :frozen], np.broadcast_to(theta[:frozen], (n_members, frozen))) and not _same(got[0], got[1])
        seen.append(got)
        # the whole device layout, its padding included: the same launch on a population loaded through set_params
        other.set_params(want)
        outs = []
        for p in (pop, other):
            res = p.act(obs, 64, "greedy", want_out)
            p.sync()
            outs.append({key: _download(val.__cuda_array_interface__["data"][0], np.dtype(val.__cuda_array_interface__["typestr"]),
                                        int(np.prod(val.__cuda_array_interface__["shape"]))) for key, val in res.items()})
        for key in outs[0]:
            assert _same(outs[0][key], outs[1][key]), (generation, key)
        assert np.isfinite(outs[0]["logits"]).all()
        assert es.generation == generation                  # ask leaves the counter alone
    assert not _same(seen[0], seen[1])
    # the low word alone (generation 3) asks other members than 2^32 + 3 did
    es.set_state(None, 3)
    es.ask(pop)
    assert not _same(_members(pop), seen[1]) and _same(_members(pop), P.es_ask_ref(theta, sigma, frozen, n_members, SEED, 3))
    for x in (es, pop, other):
        x.close()


def _fitness_cases(n_members, rng):
    if n_members == 2:
        return [np.array(f) for f in ([1.0, 1.0], [np.nan, np.nan], [-np.inf, np.inf], [0.25, -3.0], [np.nan, 0.0])]
    f = rng.normal(size=n_members)
    f[7] = f[3]                                # a tie
    f[10] = f[11] = np.nan                     # a NaN pair
    f[20], f[21], f[40], f[41 + 64] = np.inf, -np.inf, np.inf, np.nan
    return [f, rng.normal(size=n_members), np.zeros(n_members)] + beyond_one_tile(n_members, rng)


@pytest.mark.parametrize("n_members", [2, 130, 256, 258, 600])
def test_tell_moves_theta_as_the_definition_does(n_members):
    import torch
    spec, theta0 = seeded_policy((16,), "relu", None, seed=9)
    sigma, lr, frozen = 0.1, 0.05, 10
    es = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=sigma, lr=lr, seed=SEED, frozen=frozen)
    theta = theta0.astype(np.float64)
    generation = 0
    for round_, f in enumerate(_fitness_cases(n_members, np.random.default_rng(n_members))):
        if round_ == 1:
            generation = LATE
            es.set_state(None, generation)
        d_f = torch.from_numpy(f).cuda()
        torch.cuda.synchronize()
        if round_ % 2:
            es.tell(d_f.data_ptr())                        # a raw pointer ...
        else:
            es.tell(d_f)                                   # ... or anything with __cuda_array_interface__
        want = P.es_tell_ref(theta, f, sigma, lr, frozen, SEED, generation)
        got = es.theta
        assert _same(got, want), round_
        assert _same(got[:frozen], theta0[:frozen].astype(np.float64)) and np.isfinite(got).all()
        generation += 1
        assert es.generation == generation
        theta = want
    assert not _same(theta, theta0.astype(np.float64))
    # frozen = every parameter: nothing moves, the generation still advances; frozen = 0: everything may
    for frozen in (P.n_params(spec), 0):
        es2 = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=sigma, lr=lr, seed=1, frozen=frozen)
        f = np.random.default_rng(5).normal(size=n_members)
        es2.tell(torch.from_numpy(f).cuda())
        assert _same(es2.theta, P.es_tell_ref(theta0, f, sigma, lr, frozen, 1, 0)) and es2.generation == 1
        es2.close()
    with pytest.raises(ValueError):
        es.tell(torch.zeros(n_members + 2, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        es.tell(torch.zeros(n_members, dtype=torch.float32, device="cuda"))
    es.close()


TAIL_IDS = ["seed%d-j%d" % row[:2] for row in tail_rows()]


def _tail_strategy(row, n_members=2, **kw):
    """spec (16,) relu, theta = 0 behind the ten input entries, sigma = 1 and lr = P, so that c = lr / (P * sigma) = 1"""
    import torch
    spec, theta0 = seeded_policy((16,), "relu", None, seed=23)
    theta0[10:] = 0.0
    es = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=1.0, lr=float(n_members), seed=row[0], frozen=10, **kw)
    fitness = np.linspace(1.0, 0.0, n_members)                 # descending: member 0, the + z one of pair 0, is the best
    d_f = torch.from_numpy(fitness).cuda()
    torch.cuda.synchronize()
    return spec, theta0.astype(np.float64), es, fitness, d_f


@pytest.mark.parametrize("row", tail_rows(), ids=TAIL_IDS)
def test_the_far_tail_of_the_inverse_normal_reaches_ask_and_tell(row):
    """z(0, 0, j) of the row's seed comes from the r > 5 branch of es_inverse_normal, which no test reaches by chance.  ask: the
    two members are the restatement's, column j the float of +-z.  tell with fitness [1, 0]: w_0 = 1, c = 1 and the tree adds
    +0.0 alone, so theta_j IS the recorded z - with no restatement in between."""
    seed, j, _, z = row
    spec, theta0, es, fitness, d_f = _tail_strategy(row)
    pop = P.PolicyPopulation(spec, n_members=2)
    es.ask(pop)
    got = _members(pop)
    assert _same(got, P.es_ask_ref(theta0, 1.0, 10, 2, seed, 0))
    assert _same(got[:, j], np.array([z, -z]).astype(np.float32)) and abs(z) > 6.6579046435
    es.tell(d_f)
    theta = es.theta
    assert _same(theta, P.es_tell_ref(theta0, fitness, 1.0, 2.0, 10, seed, 0))
    assert _same(theta[j], np.float64(z)), (float(theta[j]).hex(), float(z).hex())
    assert np.abs(np.delete(theta, j)[10:]).max() < 6.0 and es.generation == 1     # (the one wild draw is the recorded one)
    assert _same(theta[:10], theta0[:10])
    es.close()
    pop.close()


@pytest.mark.parametrize("n_members", [2, 4])
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("row", tail_rows(), ids=TAIL_IDS)
def test_the_far_tail_goes_through_the_step_size_rule_and_adam(row, optimizer, n_members):
    """The same draw under BSK_ES_SIGMA_PGPE (es_tell_sigma_kernel / es_tell_adam_sigma_kernel).  Two members have
    q_0 = u_0 + u_1 = 0 and the vector cannot move; FOUR have q_0 = 2 / 3, and there z * z - 1, about 45, is the largest term the
    rule ever sees: parameter j runs into the max_change clamp and then into sigma_max."""
    seed, j, _, z = row
    adam = dict(optimizer="adam", beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2) if optimizer == "adam" else {}
    rule = (4.0, 0.2, 0.5, 1.1)
    spec, theta0, es, fitness, d_f = _tail_strategy(row, n_members, sigma_adapt="pgpe", lr_sigma=rule[0], sigma_max_change=rule[1],
                                                    sigma_min=rule[2], sigma_max=rule[3], **adam)
    n = theta0.size
    state = (np.zeros(n), np.zeros(n), np.ones(2), 0.9, 0.999, 1e-8, 1e-2) if optimizer == "adam" else None
    es.tell(d_f)
    want = P.es_tell_pgpe_ref(theta0, np.ones(n), fitness, float(n_members), 10, seed, 0, *rule, adam=state)
    got = (es.theta, es.sigma_vector) + (es.moments if optimizer == "adam" else ())
    for g, w, name in zip(got, want, ("theta", "sigma", "m", "v", "beta_pow")):
        assert _same(g, w), name
    assert np.isfinite(got[0]).all() and got[0][j] != 0.0
    if n_members == 2:
        assert _same(got[1], np.ones(n))
        if optimizer == "sgd":
            assert _same(got[0][j], np.float64(z))             # lr / (Pd * sg) = 1
    else:
        # (elsewhere r is 2 / 3 of z_0 ** 2 - z_1 ** 2 of two ordinary draws: some entries stop at the lower clamp, some move freely)
        assert got[1][j] == 1.1 and (got[1][10:] == 0.8).any() and ((got[1][10:] > 0.8) & (got[1][10:] < 1.1)).any()
    es.close()


@pytest.mark.parametrize("row", tail_rows(), ids=TAIL_IDS)
def test_the_far_tail_goes_through_adam(row):
    """... and under Adam with the one sigma (es_tell_adam_kernel): g_j = z / 2 - weight_decay * 0 is the first gradient Adam sees"""
    seed, j, _, z = row
    _, theta0, es, fitness, d_f = _tail_strategy(row, optimizer="adam", beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)
    n = theta0.size
    es.tell(d_f)
    want = P.es_tell_adam_ref(theta0, np.zeros(n), np.zeros(n), np.ones(2), fitness, 1.0, 2.0, 10, seed, 0, 0.9, 0.999, 1e-8, 1e-2)
    got = (es.theta,) + es.moments
    for g, w, name in zip(got, want, ("theta", "m", "v", "beta_pow")):
        assert _same(g, w), name
    assert np.isfinite(got[0]).all() and _same(got[1][j], (1.0 - 0.9) * (0.5 * np.float64(z)))
    es.close()


def _propagator(n, ic, stream=None):
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    cfg.max_length = 6
    p = BatchedPropagator(cfg, n, stream=stream)
    p.set_ic_pool(sample_ic_batch(41, 4, seed=15))
    p.reset(ic)
    p.step(np.zeros(n, np.int32), 1)
    return p


def test_generations_run_on_the_device_and_replay_from_a_hip_graph():
    import torch
    n_members, E, T, k, gamma = 4, 64, 8, 1, 0.99
    n = n_members * E
    spec, theta0 = seeded_policy((16,), "tanh", None, seed=5)
    sigma, lr, frozen, seed = 0.1, 0.05, 10, 3
    ic = sample_ic_batch(n, 4, seed=29)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        # the reference: the same three generations composed on the host from pieces that already ship and the restatement
        prop = _propagator(n, ic, side.cuda_stream)
        pop = P.PolicyPopulation(spec, n_members=n_members)
        d_fit = torch.full((n_members,), -7.0, dtype=torch.float64, device="cuda")
        theta, want = theta0.astype(np.float64), []
        for g in range(3):
            pop.set_params(P.es_ask_ref(theta, sigma, frozen, n_members, seed, g))
            prop.reset_from_pool_device(None)
            pop.rollout_device(prop, T, k, "greedy", gamma, d_fitness=d_fit.data_ptr())
            prop.sync()
            fitness = d_fit.cpu().numpy()
            theta = P.es_tell_ref(theta, fitness, sigma, lr, frozen, seed, g)
            want.append((theta, fitness))
        assert np.isfinite(want[2][1]).all() and not _same(want[0][1], want[1][1]) and not _same(want[0][0], want[2][0])
        prop.close()
        pop.close()

        def make():
            prop = _propagator(n, ic, side.cuda_stream)
            pop = P.PolicyPopulation(spec, n_members=n_members)
            es = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=sigma, lr=lr, seed=seed, frozen=frozen)
            return prop, pop, es

        def state(es):
            theta = es.theta                                # (synchronises the device)
            return theta, _download(es.fitness_buffer().ptr, np.float64, n_members)

        prop, pop, es = make()
        for g in range(3):
            c0 = BatchedPropagator.debug_counters()
            es.run_generation(prop, pop, T, k, "greedy", gamma)
            if g:
                assert BatchedPropagator.debug_counters() == c0      # no copy, no synchronisation
            got = state(es)
            assert _same(got[0], want[g][0]) and _same(got[1], want[g][1]), g
            assert es.generation == g + 1
        for x in (prop, pop, es):
            x.close()

        # captured once behind a warming call, replayed twice: generations two and three of the run above
        prop, pop, es = make()
        es.run_generation(prop, pop, T, k, "greedy", gamma)
        prop.sync()
        assert _same(state(es)[0], want[0][0])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            es.run_generation(prop, pop, T, k, "greedy", gamma)
        for g in (1, 2):
            c0 = BatchedPropagator.debug_counters()
            graph.replay()
            torch.cuda.synchronize()
            assert BatchedPropagator.debug_counters() == c0
            got = state(es)
            assert _same(got[0], want[g][0]) and _same(got[1], want[g][1]), g
            assert es.generation == g + 1
        for x in (prop, pop, es):
            x.close()


def test_twenty_generations_descend_as_the_numpy_loop_does():
    import torch
    n_members, sigma, lr, frozen, seed = 16, 0.1, 0.05, 10, 11
    spec, theta0 = seeded_policy((16,), "relu", None, seed=13)
    n = P.n_params(spec)
    target = np.concatenate([theta0[:frozen].astype(np.float64), np.random.default_rng(4).normal(size=n - frozen)])
    d_target = torch.from_numpy(target).cuda()
    es = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=sigma, lr=lr, seed=seed, frozen=frozen)
    pop = P.PolicyPopulation(spec, n_members=n_members)
    theta = theta0.astype(np.float64)
    for g in range(20):
        es.ask(pop)
        members = _members(pop)
        want = P.es_ask_ref(theta, sigma, frozen, n_members, seed, g)
        assert _same(members, want), g
        d_fitness = -((torch.from_numpy(members).cuda().double() - d_target) ** 2).sum(dim=1)
        fitness = -((want.astype(np.float64) - target) ** 2).sum(axis=1)
        assert np.array_equal(P.centred_ranks(d_fitness.cpu().numpy()), P.centred_ranks(fitness)), g
        torch.cuda.synchronize()
        es.tell(d_fitness)
        theta = P.es_tell_ref(theta, fitness, sigma, lr, frozen, seed, g)
        assert _same(es.theta, theta), g
    start, end = np.linalg.norm(theta0 - target), np.linalg.norm(theta - target)
    assert end < start and es.generation == 20 and _same(theta[:frozen], theta0[:frozen].astype(np.float64))
    es.close()
    pop.close()


def test_refusals_come_before_any_launch():
    import torch
    lib = _lib.load()
    n_members = 4
    spec, theta0 = seeded_policy((16,), "relu", None, seed=21)
    cs, h = P.c_spec(spec), ctypes.c_void_p()
    np_ = P.n_params(spec)
    nan, inf = float("nan"), float("inf")
    for args in ((3, 0.1, 0.05, 10), (1, 0.1, 0.05, 10), (0, 0.1, 0.05, 10), (-2, 0.1, 0.05, 10), (65538, 0.1, 0.05, 10),
                 (4, 0.0, 0.05, 10), (4, -0.1, 0.05, 10), (4, nan, 0.05, 10), (4, inf, 0.05, 10), (4, 0.1, nan, 10), (4, 0.1, inf, 10),
                 (4, 0.1, -inf, 10), (4, 0.1, 0.05, -1), (4, 0.1, 0.05, np_ + 1)):
        assert lib.bsk_es_create(ctypes.byref(cs), args[0], theta0.ctypes.data, args[1], args[2], args[3], 0, 0, ctypes.byref(h)) == -1, args
        assert lib.bsk_last_error() and not h.value
    assert lib.bsk_es_create(None, 4, theta0.ctypes.data, 0.1, 0.05, 10, 0, 0, ctypes.byref(h)) == -1
    assert lib.bsk_es_create(ctypes.byref(cs), 4, theta0.ctypes.data, 0.1, 0.05, 10, 0, 0, None) == -1
    bad = P.c_spec(spec)
    bad.hidden[0] = 17
    assert lib.bsk_es_create(ctypes.byref(bad), 3, theta0.ctypes.data, 0.1, 0.05, 10, 0, 0, ctypes.byref(h)) == -1     # the spec comes first
    assert b"bsk_policy_spec" in lib.bsk_last_error()
    with pytest.raises(_lib.BskGpuUnavailable):
        P.DeviceEvolutionStrategy(spec, theta0, n_members, device=_hip.device_count())
    with pytest.raises(ValueError):
        P.DeviceEvolutionStrategy(spec, theta0[:-1], n_members)

    es = P.DeviceEvolutionStrategy(spec, theta0, n_members, seed=2)
    sentinel = np.full((n_members, np_), 3.0, np.float32)
    pop = P.PolicyPopulation(spec, sentinel)
    fewer = P.PolicyPopulation(spec, np.full((2, np_), 3.0, np.float32))
    spec_w, _ = seeded_policy((32,), "relu", None, seed=21)
    wider = P.PolicyPopulation(spec_w, np.full((n_members, P.n_params(spec_w)), 3.0, np.float32))
    spec_t, _ = seeded_policy((16,), "tanh", None, seed=21)                 # the same shapes under another activation
    tanh = P.PolicyPopulation(spec_t, sentinel)
    spec_v, _ = seeded_policy((16,), "relu", (16,), seed=21)
    valued = P.PolicyPopulation(spec_v, np.full((n_members, P.n_params(spec_v)), 3.0, np.float32))
    d_fit = torch.zeros(n_members, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    c0 = BatchedPropagator.debug_counters()
    e = es._handle()
    for args in ((None, pop._handle()), (e, None), (e, fewer._handle()), (e, wider._handle()), (e, tanh._handle()), (e, valued._handle())):
        assert lib.bsk_es_ask(*args, None) == -1, args
        assert lib.bsk_last_error()
    assert b"spec" in lib.bsk_last_error()
    assert lib.bsk_es_tell(e, None, None) == -1 and lib.bsk_es_tell(None, d_fit.data_ptr(), None) == -1
    assert lib.bsk_es_get_state(None, None, None) == -1 and lib.bsk_es_set_state(None, None, 0) == -1
    assert BatchedPropagator.debug_counters() == c0
    others = [fewer, wider, tanh, valued]
    if _hip.device_count() > 1:
        far = P.PolicyPopulation(spec, sentinel, device=1)
        assert lib.bsk_es_ask(e, far._handle(), None) == -1 and b"different devices" in lib.bsk_last_error()
        others.append(far)
    torch.cuda.synchronize()
    for p in [pop] + others:                                 # nothing was launched: every member is the sentinel still
        assert all((p.member(m) == 3.0).all() for m in range(p.n_members))
    assert _same(es.theta, theta0.astype(np.float64)) and es.generation == 0
    # ... and the same calls with legal arguments do run
    es.ask(pop)
    es.tell(d_fit)
    assert _same(_members(pop), P.es_ask_ref(theta0, 0.1, 10, n_members, 2, 0)) and es.generation == 1
    for x in [es, pop] + others:
        x.close()
    with pytest.raises(RuntimeError):
        es.ask(pop)


def test_c_consumer_prints_the_python_bindings_theta(tmp_path):
    """tests/c_abi/c_abi_es.c: bsk_es_create / _ask / _tell / _get_state from plain C99 around bsk_population_rollout, two
    generations; its printout equals the Python binding's"""
    exe = build_c_consumer(tmp_path, "c_abi_es")
    n_members, E = 4, 64
    n = n_members * E
    ic = sample_ic_batch(n, 4, seed=53)
    spec, theta0 = seeded_policy((16,), "relu", None, seed=97)
    ic.tofile(tmp_path / "ic.bin")
    theta0.tofile(tmp_path / "theta.bin")
    got = subprocess.check_output([str(exe), str(tmp_path / "ic.bin"), str(n), str(tmp_path / "theta.bin"), str(n_members)]).decode().split()
    es = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=0.1, lr=0.05, seed=SEED, frozen=10)
    pop = P.PolicyPopulation(spec, n_members=n_members)
    d_fit = _hip.DeviceBuffer(8 * n_members, 0)
    want = []
    for _ in range(2):
        prop = BatchedPropagator(default_config(4, GRAV_PM_J2), n)
        prop.reset(ic)
        prop.step(np.zeros(n, np.int32), 5)
        es.ask(pop, prop.stream_ptr())
        pop.rollout_device(prop, 6, 5, "greedy", 0.97, d_fitness=d_fit.ptr)
        es.tell(d_fit.ptr, prop.stream_ptr())
        prop.sync()
        want += _download(d_fit.ptr, np.float64, n_members).tolist()
        prop.close()
    want += es.theta.tolist() + [float(es.generation)]
    assert len(got) == len(want) == 2 * n_members + P.n_params(spec) + 1
    assert [float(v) for v in got] == want
    assert want[-1] == 2.0 and want[:n_members] != want[n_members:2 * n_members]
    d_fit.free()
    es.close()
    pop.close()
