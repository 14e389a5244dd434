"""GPU: validation of the evolution strategy's centre on fixed episodes, inside each generation (bsk_es_set_validation and its
accessors, bsk_population_set_obs_stats_members; es_center_kernel, es_validate_kernel and es_val_best_kernel in csrc/bsk_es.hip;
contract in include/bskgpu.h).

Every check is an EQUALITY of bits: against the numpy restatements (policy.es_center_ref / es_validate_ref, which
tests/test_es_validation_host.py holds to an operation-by-operation restatement), against a twin optimiser without validation, or
against an independent evaluation of the centre - no tolerance anywhere.  One exception the definition makes itself: which NaN
f_c becomes when a NaN, or +inf and -inf, are among the V values is not defined, so that column compares as "the same bits, or a
NaN in both".
Shapes: a bare J2 handle with four wheels and an auto-reset pool of 41 slots, K = 2 sub-steps, 6 env steps of episodes at most 4
long (so every env restarts once inside a rollout, by the per-env rule), E = 64; P = 4 with V = 1 is one pair per lane of the
ranking and one validation member, P = 130 with V = 3 gives the one-wave reductions lanes with two and three terms and the sum over
v more than one term; seed 2^33 + 5 and generation 2^32 + 3 catch a dropped high word.
"""
import ctypes
import subprocess

import numpy as np
import pytest

from _device_bits import bits as _bits, build_c_consumer, download as _download, same as _same
from _policy_bounds import seeded_policy
from basilisk_env_amd import _hip, _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch

pytestmark = pytest.mark.gpu

SEED, LATE = 2 ** 33 + 5, 2 ** 32 + 3
SPECS = {"relu16": ((16,), "relu", None), "tanh16x32v16": ((16, 32), "tanh", (16,))}
SHAPES = [(4, 1), (130, 3)]
# Only action 0 earns a reward on this handle.  Under these seeds of seeded_policy the greedy action is 0 for roughly half of the
# observations, of the centre and of a member sigma = 0.1 away: the rollouts' fitness values are no zeros, and they differ.
POLICY_SEED = {"relu16": 33, "tanh16x32v16": 14}
PGPE = dict(sigma_adapt="pgpe", lr_sigma=4.0, sigma_max_change=0.2, sigma_min=0.05, sigma_max=0.2)
ADAM = dict(optimizer="adam", beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2)
RULES = {"sgd-fixed": {}, "adam-fixed": ADAM, "sgd-pgpe": PGPE, "adam-pgpe": dict(ADAM, **PGPE)}
NAN, INF = float("nan"), float("inf")
N_POOL, E, T, K, GAMMA = 41, 64, 6, 2, 0.97


def _same_or_nan(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    ok = _bits(a) == _bits(b)
    if a.dtype.kind == "f":
        ok = ok | (np.isnan(a) & np.isnan(b))
    return bool(np.all(ok))


def _make(spec, theta0, n_members, rule, frozen=10, lr=0.05, seed=SEED, **kw):
    args = dict(RULES[rule])
    args.update(kw)
    return P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=0.1, lr=lr, seed=seed, frozen=frozen, **args)


def _training(es):
    """everything training leaves on the optimiser -> dict of arrays"""
    out = {"theta": es.theta, "generation": np.uint64(es.generation)}
    if es.optimizer == "adam":
        out.update(zip(("m", "v", "beta_pow"), es.moments))
    if es.sigma_adapt is not None:
        out["sigma"] = es.sigma_vector
    if es.log_capacity:
        out.update(("log." + k, v) for k, v in es.training_log().items())
        out.update(zip(("best.params", "best.fitness", "best.generation", "best.member"), (np.asarray(x) for x in es.best)))
    return out


def _assert_same_training(got, want, where=""):
    assert sorted(got) == sorted(want)
    for key in want:
        assert _same_or_nan(got[key], want[key]), (where, key)


def _raw_validation(es):
    C = es.validation_capacity
    gen, rows = np.empty(C, np.uint64), np.empty((C, 4), np.float64)
    _lib.check(es._lib.bsk_es_get_validation_log(es._handle(), gen.ctypes.data, rows.ctypes.data))
    return gen, rows


def _assert_validation_is(es, ref, where=""):
    """ring and validated champion against es_validate_ref's state; f_c as 'the same bits, or a NaN in both'"""
    gen, rows = _raw_validation(es)
    assert np.array_equal(gen, ref["gen"]), where
    assert _same_or_nan(rows[:, 0], ref["rows"][:, 0]) and _same(rows[:, 1:], ref["rows"][:, 1:]), (where, rows, ref["rows"])
    params, fitness, generation = es.validated_best
    assert _same(params, ref["best_params"]) and _same_or_nan(np.float64(fitness), np.float64(ref["best_fitness"])), where
    assert generation == ref["best_generation"], where


def _propagator(n, ic, pool, stream=None, max_length=4):
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    cfg.max_length = max_length
    p = BatchedPropagator(cfg, n, stream=stream)
    p.set_ic_pool(pool)
    p.reset(np.ascontiguousarray(ic[:, :n]))
    p.step(np.zeros(n, np.int32), 1)
    return p


def _planted(theta0, frozen):
    """theta with a -0.0 among the frozen and among the moving parameters, and values that are no floats"""
    theta = theta0.astype(np.float64) + np.float64(2.0) ** -30
    theta[3] = -0.0
    theta[frozen + 7] = -0.0
    return theta


@pytest.mark.parametrize("pgpe", [False, True])
@pytest.mark.parametrize("n_members,n_val", SHAPES)
@pytest.mark.parametrize("which", sorted(SPECS))
def test_ask_writes_the_centre_behind_the_members_it_wrote_before(which, n_members, n_val, pgpe):
    hidden, activation, value_hidden = SPECS[which]
    spec, theta0 = seeded_policy(hidden, activation, value_hidden, seed=7)
    rule, frozen = ("sgd-pgpe" if pgpe else "sgd-fixed"), 10
    es, twin = _make(spec, theta0, n_members, rule, validation_members=n_val), _make(spec, theta0, n_members, rule)
    assert es.members_total == n_members + n_val and twin.members_total == n_members and es.validation_capacity == 64
    theta = _planted(theta0, frozen)
    for opt in (es, twin):
        opt.set_state(theta, LATE)
        if pgpe:
            opt.set_sigma(np.random.default_rng(77).uniform(0.06, 0.18, size=theta0.size))
    sentinel = np.full((n_members + n_val, theta0.size), 3.0, np.float32)
    pop, small = P.PolicyPopulation(spec, sentinel), P.PolicyPopulation(spec, sentinel[:n_members])
    c0 = BatchedPropagator.debug_counters()
    es.ask(pop)
    twin.ask(small)
    assert BatchedPropagator.debug_counters() == c0                  # two launches and one: no copy, no synchronisation
    centre = P.es_center_ref(theta)
    assert _same(centre, theta.astype(np.float32)) and np.signbit(centre[3]) and np.signbit(centre[frozen + 7])
    for v in range(n_val):
        assert _same(pop.member(n_members + v), centre), v
    want = P.es_ask_sigma_ref(theta, es.sigma_vector, frozen, n_members, SEED, LATE) if pgpe else P.es_ask_ref(theta, 0.1, frozen, n_members, SEED, LATE)
    for m in sorted({0, 1, 2, n_members // 2, n_members - 2, n_members - 1}):
        assert _same(pop.member(m), small.member(m)) and _same(pop.member(m), want[m]), m
    assert not _same(pop.member(0), centre) and not _same(pop.member(n_members - 1), centre)
    for x in (es, twin, pop, small):
        x.close()


def _validation_script(n_val):
    """the V validation values of six tells: take; a NaN among them; a tie with the incumbent (V = 3: the same values in the
    other order, which sum lower, then the tie); higher; +inf; +inf and -inf (V = 1: -inf)"""
    if n_val == 1:
        return [[0.5], [NAN], [0.5], [0.75], [INF], [-INF]]
    return [[1.0, 1.0, 2.0 ** 53], [1.0, NAN, 1.0], [2.0 ** 53, 1.0, 1.0], [1.0, 1.0, 2.0 ** 53], [INF, 1.0, 2.0], [INF, -INF, 0.0]]


def _training_fitness(n_members, rng, round_):
    f = rng.normal(size=n_members)
    if n_members == 4:
        return [f, np.array([1.0, 1.0, NAN, -INF]), f * 2.0, np.array([INF, 0.0, -0.0, NAN]), f - 1.0, np.full(4, NAN)][round_]
    if round_ == 1:
        f[7] = f[3]                                # a tie
        f[10] = f[11] = np.nan                     # a NaN pair
        f[20], f[21], f[40], f[41 + 64] = np.inf, -np.inf, np.inf, np.nan
    elif round_ == 3:
        f[:] = np.nan
    return f


@pytest.mark.parametrize("log", [False, True])
@pytest.mark.parametrize("n_members,n_val", SHAPES)
@pytest.mark.parametrize("rule", sorted(RULES))
def test_tell_scores_the_centre_by_the_definition_and_trains_as_its_twin(rule, n_members, n_val, log):
    import torch
    spec, theta0 = seeded_policy((16,), "relu", None, seed=9)
    C, frozen = 3, 10
    kw = dict(log_capacity=4) if log else {}
    es, twin = _make(spec, theta0, n_members, rule, **kw), _make(spec, theta0, n_members, rule, **kw)
    rng = np.random.default_rng(n_members + 7 * log)
    total = n_members + n_val
    lens = d_lens = None
    if log:
        es.set_validation(n_val, C, 11)                       # the log's own length buffer: zeros, so L_c = +0.0
        assert es._val_len == es._log_len
    else:
        lens = (rng.integers(1, 7, size=total) + rng.integers(0, 64, size=total) / 64.0).astype(np.float64)
        d_lens = torch.from_numpy(lens).cuda()
        torch.cuda.synchronize()
        es.set_validation(n_val, C, 11, d_lens)
    assert _same(_download(es.validation_epochs_ptr(), np.uint64, n_val), np.arange(11, 11 + n_val, dtype=np.uint64))
    ref = P.es_validation_state(n_val, C, theta0.size, 11)
    _assert_validation_is(es, ref, "empty")
    for opt in (es, twin):
        opt.set_state(_planted(theta0, frozen), LATE)
    _assert_validation_is(es, ref, "set_state leaves it alone")
    takes = []
    for round_, val in enumerate(_validation_script(n_val)):
        generation = LATE + round_
        f = np.concatenate([_training_fitness(n_members, rng, round_), val])
        theta = es.theta
        d_f = torch.from_numpy(f).cuda()
        d_head = torch.from_numpy(f[:n_members].copy()).cuda()
        torch.cuda.synchronize()
        c0 = BatchedPropagator.debug_counters()
        es.tell(d_f)
        twin.tell(d_head)
        assert BatchedPropagator.debug_counters() == c0            # launches only: no copy, no synchronisation
        ref = P.es_validate_ref(ref, f, lens, generation, theta)
        takes.append(ref["take"])
        _assert_validation_is(es, ref, round_)
        _assert_same_training(_training(es), _training(twin), round_)
        assert es.generation == generation + 1
    assert takes == ([1, 0, 0, 1, 1, 0] if n_val == 1 else [1, 0, 0, 0, 1, 0])
    table = es.validation_log()
    assert table["generation"].tolist() == [LATE + 3, LATE + 4, LATE + 5] and table["take"].tolist() == takes[3:]
    assert table["members"].tolist() == [n_val] * 3 and (LATE % C, 3 % C) == (1, 0)
    if lens is not None:
        assert (table["mean_len"] > 0.0).all()
    # tell refuses P values now, and the twin P + V
    with pytest.raises(ValueError):
        es.tell(d_head)
    with pytest.raises(ValueError):
        twin.tell(d_f)
    for x in (es, twin):
        x.close()


def _world(spec, theta0, n_members, n_val, rule, pool, ic, stream=None, stats_cap=None, **kw):
    total = n_members + n_val
    prop = _propagator(total * E, ic, pool, stream)
    pop = P.PolicyPopulation(spec, n_members=total)
    es = _make(spec, theta0, n_members, rule, validation_members=n_val, **kw)
    es.set_state(None, LATE)
    stats = P.ObsStats(stats_cap) if stats_cap else None
    return prop, pop, es, stats


def _close(*objs):
    for x in objs:
        if x is not None:
            x.close()


@pytest.mark.parametrize("mode", ["greedy", "sample"])
@pytest.mark.parametrize("with_stats", [False, True])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("n_members,n_val,which", [(4, 1, "tanh16x32v16"), (130, 3, "relu16")])
def test_training_with_validation_is_training_without_it(n_members, n_val, which, shared, with_stats, mode):
    hidden, activation, value_hidden = SPECS[which]
    spec, theta0 = seeded_policy(hidden, activation, value_hidden, seed=POLICY_SEED[which])
    pool, ic = sample_ic_batch(N_POOL, 4, seed=15), sample_ic_batch((n_members + n_val) * E, 4, seed=29)
    cap = n_members * E if with_stats else None
    a = _world(spec, theta0, n_members, n_val, "adam-pgpe", pool, ic, stats_cap=cap, log_capacity=8)
    b = _world(spec, theta0, n_members, 0, "adam-pgpe", pool, ic, stats_cap=cap, log_capacity=8)
    for (prop, pop, es, stats) in (a, b):
        pop.set_rng(SEED, 0)
    for g in range(5):
        for (prop, pop, es, stats) in (a, b):
            c0 = BatchedPropagator.debug_counters()
            es.run_generation(prop, pop, T, K, mode, GAMMA, shared_episodes=shared, obs_stats=stats)
            if g:
                assert BatchedPropagator.debug_counters() == c0      # no copy, no synchronisation after the warming call
    for (prop, pop, es, stats) in (a, b):
        prop.sync()
    _assert_same_training(_training(a[2]), _training(b[2]))
    fit_a, fit_b = _download(a[2].fitness_buffer().ptr, np.float64, n_members + n_val), _download(b[2].fitness_buffer().ptr, np.float64, n_members)
    assert _same(fit_a[:n_members], fit_b) and np.isfinite(fit_a).all() and len(set(fit_a.tolist())) > 1
    assert a[1].get_rng() == b[1].get_rng()
    if with_stats:
        (part_a, cnt_a), (part_b, cnt_b) = a[3].state, b[3].state
        assert _same(part_a, part_b) and np.array_equal(cnt_a, cnt_b) and a[3].count == b[3].count > 0
        assert getattr(a[1], "_stats", None) is None
    table = a[2].validation_log()
    assert table["generation"].tolist() == [LATE + g for g in range(5)] and table["members"].tolist() == [n_val] * 5
    assert np.isfinite(table["fitness"]).all() and (table["mean_len"] >= 1.0).all() and (table["mean_len"] <= T).all()
    assert table["take"][0] == 1 and _same(np.float64(a[2].validated_best[1]), table["fitness"].max())
    _close(*a)
    _close(*b)


@pytest.mark.parametrize("n_members,n_val,which", [(4, 1, "tanh16x32v16"), (130, 3, "relu16")])
def test_the_centre_meets_the_same_episodes_in_every_generation(n_members, n_val, which):
    hidden, activation, value_hidden = SPECS[which]
    spec, theta0 = seeded_policy(hidden, activation, value_hidden, seed=POLICY_SEED[which])
    pool, ic = sample_ic_batch(N_POOL, 4, seed=15), sample_ic_batch((n_members + n_val) * E, 4, seed=29)
    prop, pop, es, _ = _world(spec, theta0, n_members, n_val, "sgd-fixed", pool, ic, lr=0.0)
    theta = es.theta
    fits = []
    for g in range(4):
        es.run_generation(prop, pop, T, K, "greedy", GAMMA, shared_episodes=True)
        prop.sync()
        fits.append(_download(es.fitness_buffer().ptr, np.float64, n_members + n_val))
    assert _same(es.theta, theta) and es.generation == LATE + 4       # lr = 0: the centre stays
    table = es.validation_log()
    assert len(set(_bits(table["fitness"]).tolist())) == 1 and table["take"].tolist() == [1, 0, 0, 0]
    for g in range(1, 4):
        assert _same(fits[g][n_members:], fits[0][n_members:]) and not _same(fits[g][:n_members], fits[0][:n_members])
    # an independent evaluation: the centre alone, on a handle of E envs, restarted under validation member v's epoch word
    one = P.PolicyPopulation(spec, P.es_center_ref(theta)[None, :])
    alone = _propagator(E, ic, pool)
    d_fit = _hip.DeviceBuffer(8, 0)
    scores = []
    for v in range(n_val):
        alone.reset_from_pool_shared(E, es.validation_epochs_ptr() + 8 * v)
        one.rollout_device(alone, T, K, "greedy", GAMMA, d_fitness=d_fit.ptr)
        alone.sync()
        scores.append(_download(d_fit.ptr, np.float64, 1)[0])
    assert _same(np.array(scores), fits[0][n_members:])
    if n_val > 1:
        assert len(set(scores)) > 1                                    # (the V members meet different episodes)
    s = np.float64(scores[0])
    for v in range(1, n_val):
        s = np.float64(s + scores[v])
    assert _same(np.float64(s / np.float64(n_val)), table["fitness"][0]) and _same(np.float64(es.validated_best[1]), table["fitness"][0])
    assert _same(es.validated_best[0], P.es_center_ref(theta)) and es.validated_best[2] == LATE
    d_fit.free()
    _close(prop, pop, es, one, alone)


def test_a_replayed_graph_validates_as_the_eager_loop():
    import torch
    n_members, n_val = 4, 1
    spec, theta0 = seeded_policy((16,), "relu", None, seed=POLICY_SEED["relu16"])
    pool, ic = sample_ic_batch(N_POOL, 4, seed=15), sample_ic_batch((n_members + n_val) * E, 4, seed=29)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        def make():
            return _world(spec, theta0, n_members, n_val, "adam-pgpe", pool, ic, side.cuda_stream, stats_cap=n_members * E, log_capacity=8)

        def run(world):
            prop, pop, es, stats = world
            es.run_generation(prop, pop, T, K, "greedy", GAMMA, shared_episodes=True, obs_stats=stats)

        eager = make()
        for g in range(5):
            run(eager)
        eager[0].sync()
        want, want_val, want_best, want_stats = _training(eager[2]), _raw_validation(eager[2]), eager[2].validated_best, eager[3].state
        assert sorted(want_val[0].tolist())[:5] == [LATE + g for g in range(5)] and eager[2].generation == LATE + 5
        assert len(set(want_val[1][:, 0].tolist())) > 2              # (the centre moves, and its score with it)
        _close(*eager)

        world = make()
        run(world)                                                    # the warming call: buffers, scratch rows, masks
        world[0].sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            run(world)
        c0 = BatchedPropagator.debug_counters()
        for _ in range(4):
            graph.replay()
        torch.cuda.synchronize()
        assert BatchedPropagator.debug_counters() == c0
        _assert_same_training(_training(world[2]), want)
        gen, rows = _raw_validation(world[2])
        assert np.array_equal(gen, want_val[0]) and _same(rows, want_val[1])
        best = world[2].validated_best
        assert _same(best[0], want_best[0]) and _same(np.float64(best[1]), np.float64(want_best[1])) and best[2] == want_best[2]
        assert _same(world[3].state[0], want_stats[0]) and np.array_equal(world[3].state[1], want_stats[1])
        _close(*world)


def test_the_validated_champion_is_handed_on_and_a_checkpoint_resumes():
    import torch
    hidden, activation, value_hidden = SPECS["tanh16x32v16"]
    spec, theta0 = seeded_policy(hidden, activation, value_hidden, seed=7)
    n_members, n_val, C = 4, 3, 4
    es = _make(spec, theta0, n_members, "adam-pgpe", validation_members=n_val, validation_capacity=C, validation_epoch=5)
    es.set_state(_planted(theta0, 10), LATE)
    rng = np.random.default_rng(8)
    fs = [np.concatenate([rng.normal(size=n_members), val]) for val in ([0.25, 0.5, 0.125], [3.0, 1.0, 0.5], [0.0, 0.0, 0.0], [2.0, 4.0, 8.0])]
    thetas = []
    for f in fs[:2]:
        thetas.append(es.theta)
        es.tell(torch.from_numpy(f).cuda())
    best = es.validated_best
    assert best[1:] == (1.5, LATE + 1) and _same(best[0], P.es_center_ref(thetas[1])) and not _same(best[0], P.es_center_ref(thetas[0]))
    # the hand-off: no host in between
    sentinel = np.full((3, theta0.size), 3.0, np.float32)
    pop = P.PolicyPopulation(spec, sentinel)
    c0 = BatchedPropagator.debug_counters()
    pop.set_params_device(es.validated_best_params_ptr(), 1, 1)
    assert BatchedPropagator.debug_counters() == c0
    assert _same(pop.member(1), best[0]) and (pop.member(0) == 3.0).all() and (pop.member(2) == 3.0).all()
    # round trips, whole and one word at a time; the ring stays
    saved = dict(theta=es.theta, generation=es.generation, moments=es.moments, sigma=es.sigma_vector, best=best, ring=_raw_validation(es))
    es.set_validated_best(np.zeros(theta0.size, np.float32), -1.0, 7)
    got = es.validated_best
    assert not got[0].any() and got[1:] == (-1.0, 7)
    es.set_validated_best(fitness=NAN)
    assert np.isnan(es.validated_best[1]) and es.validated_best[2] == 7
    es.set_validated_best(*best)
    got = es.validated_best
    assert _same(got[0], best[0]) and got[1:] == best[1:]
    gen, rows = _raw_validation(es)
    assert np.array_equal(gen, saved["ring"][0]) and _same(rows, saved["ring"][1])
    resumed = _make(spec, theta0, n_members, "adam-pgpe", validation_members=n_val, validation_capacity=C, validation_epoch=5)
    resumed.set_state(saved["theta"], saved["generation"])
    resumed.set_moments(*saved["moments"])
    resumed.set_sigma(saved["sigma"])
    resumed.set_validated_best(*saved["best"])
    for f in fs[2:]:
        for opt in (es, resumed):
            opt.tell(torch.from_numpy(f).cuda())
    a, b = es.validated_best, resumed.validated_best
    assert _same(a[0], b[0]) and a[1:] == b[1:] and a[2] == LATE + 3 and _same(np.float64(a[1]), np.float64((2.0 + 4.0 + 8.0) / 3.0))
    assert _same(es.theta, resumed.theta)
    ta, tb = es.validation_log(), resumed.validation_log()
    assert ta["generation"].tolist() == [LATE + r for r in range(4)] and tb["generation"].tolist() == [LATE + 2, LATE + 3]
    for key in ta:
        assert _same(ta[key][2:], tb[key]), key
    assert ta["take"].tolist() == [1, 1, 0, 1]
    for x in (es, resumed, pop):
        x.close()


def test_what_is_refused_leaves_everything_as_it_was():
    import torch
    lib = _lib.load()
    spec, theta0 = seeded_policy((16,), "relu", None, seed=21)
    n_members, n_val = 4, 1
    es = _make(spec, theta0, n_members, "sgd-fixed", log_capacity=4)
    pop, big = P.PolicyPopulation(spec, n_members=n_members), P.PolicyPopulation(spec, n_members=n_members + n_val)
    ptr = ctypes.c_void_p()

    def is_off():
        for call in (es.validation_log, lambda: es.validated_best, es.validated_best_params_ptr, es.validation_epochs_ptr,
                     lambda: es.set_validated_best(fitness=1.0)):
            with pytest.raises(_lib.BskError) as e:
                call()
            assert e.value.code == -1 and "validation is off" in str(e.value)
        assert es.validation_members == 0 and es.members_total == n_members
        with pytest.raises(_lib.BskError):
            es.ask(big)                                              # P + V members while it is off
        es.ask(pop)

    is_off()
    h = es._handle()
    assert lib.bsk_es_set_validation(None, 1, 4, 0, None) == -1 and lib.bsk_es_set_validation(h, 17, 4, 0, None) == -1
    assert lib.bsk_es_set_validation(h, -1, 4, 0, None) == -1 and lib.bsk_es_set_validation(h, 1, 0, 0, None) == -1
    assert lib.bsk_es_validated_best_device(None, ctypes.byref(ptr)) == -1 and lib.bsk_es_get_validated_best(None, None, None, None) == -1
    assert lib.bsk_population_set_obs_stats_members(None, 1) == -1
    for bad in (0, -1, n_members + 1):
        with pytest.raises(_lib.BskError) as e:
            pop.set_obs_stats_members(bad)
        assert e.value.code == -1
    pop.set_obs_stats_members(n_members)
    pop.set_obs_stats_members(None)
    for bad in (dict(members=17), dict(members=1, capacity=0), dict(members=-1)):
        with pytest.raises(ValueError):
            es.set_validation(**bad)
    with pytest.raises(ValueError):
        es.set_validation(1, 4, 0, torch.zeros(n_members, dtype=torch.float64, device="cuda"))           # P, not P + V
    is_off()

    side = torch.cuda.Stream()
    fs = [np.array(f) for f in ([0.0, 1.0, 2.0, 3.0, 0.5], [5.0, 1.0, NAN, 3.0, 0.75], [0.5, 0.25, 4.0, 1.0])]
    with torch.cuda.stream(side):
        d_fs = [torch.from_numpy(f).cuda() for f in fs]
        torch.cuda.synchronize()
        es.set_validation(n_val)
        assert es.validation_capacity == 4 and es.members_total == n_members + n_val        # None: the log's capacity
        with pytest.raises(_lib.BskError) as e:
            es.ask(pop, side.cuda_stream)                            # P members while it is on
        assert e.value.code == -1 and "n_val" in str(e.value)
        es.ask(big, side.cuda_stream)
        es.tell(d_fs[0], side.cuda_stream)
        torch.cuda.synchronize()
        assert es.validation_log()["fitness"].tolist() == [0.5] and es.validated_best[1:] == (0.5, 0) and es.best[1:] == (3.0, 0, 3)
        theta = es.theta
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for members in (2, 0):
                with pytest.raises(_lib.BskError) as e:
                    es.set_validation(members)
                assert e.value.code == -1 and "captured" in str(e.value)
        # the refusal changed nothing: validation goes on where it was
        assert es.validation_members == n_val and _same(es.theta, theta)
        es.tell(d_fs[1], side.cuda_stream)
        torch.cuda.synchronize()
        assert es.validation_log()["fitness"].tolist() == [0.5, 0.75] and es.validated_best[1:] == (0.75, 1) and es.best[1:] == (5.0, 1, 0)
        # off again: nothing of it exists, the log and its champion are where they were, tell takes P values
        es.set_validation(0)
        is_off()
        assert es.best[1:] == (5.0, 1, 0) and es.training_log()["generation"].tolist() == [0, 1]
        es.tell(d_fs[2], side.cuda_stream)
        torch.cuda.synchronize()
        assert es.generation == 3
        # on again: empty, whatever was there before
        es.set_validation(2, 5)
        assert es.validation_log()["generation"].size == 0 and np.isnan(es.validated_best[1]) and es.validated_best[2] == P.ES_LOG_EMPTY
    for x in (es, pop, big):
        x.close()


def _small_world(members):
    """P = 2 training members and ``members`` - 2 validation members of relu16, E = 64 envs each, episodes at most 6 long
    -> (spec, theta0, propagator, population)"""
    spec, theta0 = seeded_policy((16,), "relu", None, seed=POLICY_SEED["relu16"])
    pool, ic = sample_ic_batch(N_POOL, 4, seed=15), sample_ic_batch(members * E, 4, seed=29)
    return spec, theta0, _propagator(members * E, ic, pool, max_length=6), P.PolicyPopulation(spec, n_members=members)


def _records(es):
    """everything the two records hold -> dict of arrays"""
    out = {"theta": es.theta}
    out.update(("log." + k, v) for k, v in es.training_log().items())
    out.update(("val." + k, v) for k, v in es.validation_log().items())
    out.update(zip(("best.params", "best.fitness", "best.generation", "best.member"), (np.asarray(x) for x in es.best)))
    out.update(zip(("vbest.params", "vbest.fitness", "vbest.generation"), (np.asarray(x) for x in es.validated_best)))
    return out


def test_log_and_validation_bind_one_length_buffer_in_either_order():
    """The log's length columns and the validation's read ONE device buffer - the rollout writes one - whichever of the two is
    turned on first, and whether the buffer is the optimiser's own or an array the caller bound; and the two call sequences that
    would leave them on two buffers are refused, with the optimiser left as it was."""
    import torch
    n_members, n_val, T_, K_ = 2, 1, 4, 1
    arr = torch.zeros(n_members + n_val, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    orders = {"log-val": lambda es: (es.set_log(4), es.set_validation(1)),
              "val-log": lambda es: (es.set_validation(1), es.set_log(4)),
              "val(arr)-log": lambda es: (es.set_validation(1, mean_len=arr), es.set_log(4))}
    worlds, got = {}, {}
    for name, turn_on in orders.items():
        spec, theta0, prop, pop = _small_world(n_members + n_val)
        es = _make(spec, theta0, n_members, "sgd-fixed")
        turn_on(es)
        assert es.log_capacity == 4 and es.validation_members == n_val and es.validation_capacity == (4 if name == "log-val" else 64)
        for _ in range(2):
            es.run_generation(prop, pop, T_, K_, "greedy", GAMMA, shared_episodes=True)
        prop.sync()
        worlds[name], got[name] = (prop, pop, es), _records(es)
    want = got["log-val"]
    assert want["log.generation"].tolist() == [0, 1] and want["val.generation"].tolist() == [0, 1]
    assert np.isfinite(want["log.best"]).all() and np.isfinite(want["val.fitness"]).all() and (want["log.len_sum"] >= n_members).all()
    for name in ("val-log", "val(arr)-log"):
        assert sorted(got[name]) == sorted(want)
        for key in want:
            assert _same(got[name][key], want[key]), (name, key)
    # the caller's array holds the lengths of the last generation: what the log's row summed and what the centre's row holds
    es = worlds["val(arr)-log"][2]
    lens = arr.cpu().numpy()
    fit = _download(es.fitness_buffer().ptr, np.float64, n_members + n_val)
    row = P.es_log_row_ref(fit[:n_members], lens[:n_members])
    assert (lens >= 1.0).all() and (lens <= T_).all()
    assert _same(row[6], want["log.len_sum"][1]) and _same(row[7], want["log.best_len"][1]) and _same(lens[n_members], want["val.mean_len"][1])
    # refused: another array for the log while validation is on; everything stays, and the next generation runs
    prop, pop, es = worlds["log-val"]
    other = torch.zeros(n_members + n_val, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError) as e:
        es.set_log(4, mean_len=other)
    assert str(e.value) == "mean_len: while validation is on the log reads the length buffer set_validation bound (the rollout writes one)"
    _assert_same_training(_records(es), want, "refused set_log")
    es.run_generation(prop, pop, T_, K_, "greedy", GAMMA, shared_episodes=True)
    prop.sync()
    assert es.generation == 3 and es.training_log()["generation"].tolist() == [0, 1, 2] and es.validation_log()["generation"].tolist() == [0, 1, 2]
    # refused: validation beside a log that reads a caller's array of P lengths; the log goes on as it was
    spec, theta0, prop2, pop2 = _small_world(n_members)
    es2 = _make(spec, theta0, n_members, "sgd-fixed")
    arr_p = torch.zeros(n_members, dtype=torch.float64, device="cuda")
    es2.set_log(4, mean_len=arr_p)
    with pytest.raises(ValueError) as e:
        es2.set_validation(1)
    assert str(e.value) == ("the log reads an array of P lengths the caller bound, and the rollout will write P + V: turn the log off, "
                            "give set_validation a mean_len of P + V values, then set_log the same array")
    assert es2.log_capacity == 4 and es2.validation_members == 0 and es2.members_total == n_members
    es2.run_generation(prop2, pop2, T_, K_, "greedy", GAMMA, shared_episodes=True)
    prop2.sync()
    lens_p = arr_p.cpu().numpy()
    table = es2.training_log()
    assert es2.generation == 1 and table["generation"].tolist() == [0] and (lens_p >= 1.0).all()
    assert _same(np.float64(lens_p[0] + lens_p[1]), table["len_sum"][0])
    for world in list(worlds.values()) + [(prop2, pop2, es2)]:
        _close(*world)


def test_the_two_records_move_through_their_accessors_alike():
    """get -> a fresh optimiser -> set -> get, for the log's champion and the validated one: every field's bits come back; the
    device pointers into the optimiser are four different words; and every accessor of a record that is off says so by its own
    name, before anything is copied or waited for."""
    n_members, n_val = 2, 1
    spec, theta0, prop, pop = _small_world(n_members + n_val)
    es = _make(spec, theta0, n_members, "sgd-fixed", log_capacity=4, validation_members=n_val)
    fresh = _make(spec, theta0, n_members, "sgd-fixed", log_capacity=4, validation_members=n_val)
    es.run_generation(prop, pop, 4, 1, "greedy", GAMMA, shared_episodes=True)
    prop.sync()
    for get, put, empty in ((lambda o: o.best, lambda o, x: o.set_best(*x), P.es_champion_empty(theta0.size)),
                            (lambda o: o.validated_best, lambda o, x: o.set_validated_best(*x), P.es_champion_empty(theta0.size)[:3])):
        champion, before = get(es), get(fresh)
        assert len(champion) == len(before) == len(empty)
        for x, y in zip(before, empty):
            assert _same_or_nan(np.asarray(x), np.asarray(y))
        assert champion[0].any() and np.isfinite(champion[1]) and champion[2] == 0 and (len(champion) == 3 or champion[3] in (0, 1))
        put(fresh, champion)
        for x, y in zip(get(fresh), champion):
            assert type(x) is type(y) and _same(np.asarray(x), np.asarray(y))
    # (the rows stay where they were: a champion is no row)
    assert fresh.training_log()["generation"].size == 0 and fresh.validation_log()["generation"].size == 0
    ptrs = [es.best_params_ptr(), es.validated_best_params_ptr(), es.validation_epochs_ptr(), es.generation_ptr()]
    assert all(ptrs) and len(set(ptrs)) == 4
    assert _same(_download(ptrs[0], np.float32, theta0.size), es.best[0]) and _same(_download(ptrs[1], np.float32, theta0.size), es.validated_best[0])
    off = _make(spec, theta0, n_members, "sgd-fixed")
    no_log, no_val = "the optimiser has no log (bsk_es_set_log)", "validation is off (bsk_es_set_validation)"
    refusals = [(off.training_log, "bsk_es_get_log", no_log), (lambda: off.best, "bsk_es_get_best", no_log),
                (lambda: off.set_best(fitness=1.0), "bsk_es_set_best", no_log), (off.best_params_ptr, "bsk_es_best_device", no_log),
                (off.validation_log, "bsk_es_get_validation_log", no_val), (lambda: off.validated_best, "bsk_es_get_validated_best", no_val),
                (lambda: off.set_validated_best(fitness=1.0), "bsk_es_set_validated_best", no_val),
                (off.validated_best_params_ptr, "bsk_es_validated_best_device", no_val),
                (off.validation_epochs_ptr, "bsk_es_validation_epochs_device", no_val)]
    c0 = BatchedPropagator.debug_counters()
    for call, fn, why in refusals:
        with pytest.raises(_lib.BskError) as e:
            call()
        assert e.value.code == -1 and str(e.value) == "libbskgpu error -1: %s: %s" % (fn, why)
    assert BatchedPropagator.debug_counters() == c0
    _close(prop, pop, es, fresh, off)


def test_c_consumer_prints_the_python_bindings_validation(tmp_path):
    """tests/c_abi/c_abi_es_validation.c: bsk_es_set_validation and its accessors from plain C99, two generations with one
    validation member beside two training members; its hex-float printout equals the Python binding's"""
    exe = build_c_consumer(tmp_path, "c_abi_es_validation")
    n_members, n_val = 2, 1
    n = (n_members + n_val) * E
    pool = sample_ic_batch(N_POOL, 4, seed=53)
    spec, theta0 = seeded_policy((16,), "relu", None, seed=POLICY_SEED["relu16"])
    pool.tofile(tmp_path / "pool.bin")
    theta0.tofile(tmp_path / "theta.bin")
    got = subprocess.check_output([str(exe), str(tmp_path / "pool.bin"), str(N_POOL), str(tmp_path / "theta.bin"), str(n_members), str(n_val)],
                                  timeout=120).decode().split()
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    cfg.max_length = 4
    prop = BatchedPropagator(cfg, n)
    prop.set_ic_pool(pool)
    es = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=0.1, lr=0.05, seed=SEED, frozen=10, validation_members=n_val,
                                   validation_capacity=4)
    pop = P.PolicyPopulation(spec, n_members=n_members + n_val)
    for _ in range(2):
        es.run_generation(prop, pop, T, K, "greedy", GAMMA, shared_episodes=True)
    prop.sync()
    gen, rows = _raw_validation(es)
    best = es.validated_best
    assert gen.tolist()[:2] == [0, 1] and rows[0][3] == n_val and rows[0][0] != 0.0
    want = rows[:2].reshape(-1).tolist() + [best[1], float(best[2])] + best[0].astype(np.float64).tolist() + es.theta.tolist() + [float(es.generation)]
    assert len(got) == len(want) == 8 + 2 + 2 * es.n_params + 1
    assert [float.fromhex(x).hex() for x in got] == [float(x).hex() for x in want]
    _close(prop, pop, es)
