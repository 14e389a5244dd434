"""GPU: how episodes end and which actions are used, per member, formed on the device (bsk_population_set_outcomes,
bsk_es_set_outcome_log; outcome_row_kernel / outcome_join_kernel in csrc/bsk_population.hip, es_outcome_kernel in csrc/bsk_es.hip;
contract in include/bskgpu.h).

Every check is an EQUALITY of bits: the member rows against population_outcomes_ref of the histories the same rollout recorded,
the ring against es_outcome_row_ref of the rows and fitness an eager twin produced (tests/test_outcomes_host.py holds both
restatements to a plain per-env loop), and everything else a rollout or a generation leaves against a twin that never attached
anything - no tolerance anywhere.
Shapes: a bare J2 handle with four wheels, K = 1, T = 12, [16] hidden units (and a [16] value network, so that all six histories are
recorded); (P, E) = (3, 64) is an odd member count with one
chunk per lane, (2, 128) gives every lane a chain of two.  The envs are staggered (tests/_outcome_scenario.py; looked at on the CPU
oracle with the same policies: 8 LENGTH endings per 64 envs spread over steps 0..9, 8 BATTERY at step 0, 4 WHEELS, 44 unfinished,
all three actions) and every test asserts on its own histories that the scenario did not come out empty.
"""
import subprocess

import numpy as np
import pytest

import _outcome_scenario as S
from _device_bits import build_c_consumer, download as _download, same as _same
from basilisk_env_amd import _hip, _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET
from basilisk_env_amd.simulators.dynamics import BatchedPropagator
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch

pytestmark = pytest.mark.gpu

T, K, GAMMA, N_POOL = 12, 1, 0.97, 41
HIST = (("obs", 40, np.float64, 5), ("reward", 8, np.float64, 1), ("reason", 1, np.uint8, 1), ("action", 4, np.int32, 1),
        ("logp", 4, np.float32, 1), ("value", 4, np.float32, 1))
COLS = P.OUTCOME_COLS


def _propagator(n, flags=0, stream=None, seed=14, stagger=True, max_length=S.MAX_LENGTH):
    cfg = S.config(flags, max_length)
    p = BatchedPropagator(cfg, n, stream=stream)
    if flags & FLAG_AUTO_RESET:
        p.set_ic_pool(sample_ic_batch(N_POOL, S.N_RW, seed=15))
    p.reset(sample_ic_batch(n, S.N_RW, seed=seed))
    p.step(np.zeros(n, np.int32), K)               # (the observation buffers hold a step's output, not a reset's)
    if stagger:
        S.stagger(p, cfg)
    return p


def _envs(p):
    """every buffer of the handle a rollout writes -> dict of host arrays"""
    p.sync()
    out = {"state": p.get_state()}
    out["steps"], out["ticks"] = p.get_counters()
    out["obs"], out["rew"], _, out["why"] = p.get_obs()
    v = p.device_views()
    out["done_mask"] = _download(v["done_mask"].__cuda_array_interface__["data"][0], np.uint64, (p.n_envs + 63) // 64)
    if "terminal_obs" in v:
        out["term_obs"], out["episodes"] = p.get_terminal_obs()
    return out


def _buffers(n, n_members):
    import torch
    bufs = {key: torch.zeros(T * n * size, dtype=torch.uint8, device="cuda") for key, size, _, _ in HIST}
    bufs["env_value"] = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    bufs["env_len"] = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    bufs["fitness"] = torch.full((n_members,), -7.0, dtype=torch.float64, device="cuda")
    bufs["mean_len"] = torch.full((n_members,), -7.0, dtype=torch.float64, device="cuda")
    bufs["rows"] = torch.full((n_members, COLS), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return bufs


def _host(bufs, n):
    out = {key: bufs[key].cpu().numpy().view(dt).reshape((T, 5, n) if rows == 5 else (T, n)) for key, _, dt, rows in HIST}
    for key in ("env_value", "env_len", "fitness", "mean_len", "rows"):
        out[key] = bufs[key].cpu().numpy()
    return out


def _rollout(pop, prop, bufs, mode, outcomes):
    pop.rollout_device(prop, T, K, mode, GAMMA, *(bufs[key].data_ptr() for key, _, _, _ in HIST),
                       d_env_value=bufs["env_value"].data_ptr(), d_env_len=bufs["env_len"].data_ptr(),
                       d_fitness=bufs["fitness"].data_ptr(), d_mean_len=bufs["mean_len"].data_ptr(),
                       d_outcomes=bufs["rows"].data_ptr() if outcomes else None)


def _rollout_and_its_twin(n_members, E, mode, flags):
    """one rollout with outcome rows and all six histories, and the same rollout on a twin handle and a twin population that never
    heard of outcomes -> (host results, handle buffers) of each"""
    n = n_members * E
    spec, params = S.members(n_members, (16,), seed=31, value_hidden=(16,))
    runs = []
    for outcomes in (True, False):
        prop = _propagator(n, flags)
        pop = P.PolicyPopulation(spec, params)
        pop.set_rng(77, 3)
        bufs = _buffers(n, n_members)
        _rollout(pop, prop, bufs, mode, outcomes)
        prop.sync()
        assert getattr(pop, "_outcomes", None) is None          # attached for the call only
        runs.append((_host(bufs, n), _envs(prop), pop.get_rng()))
        prop.close()
        pop.close()
    return runs


def _assert_rows_and_twin(runs, n_members, E):
    (got, envs, rng), (twin, twin_envs, twin_rng) = runs
    ref = P.population_outcomes_ref(got["reward"], got["reason"], got["action"], GAMMA, E)
    assert _same(got["rows"], ref), (got["rows"], ref)
    assert (twin["rows"] == -7.0).all()
    for key in got:
        if key != "rows":
            assert _same(got[key], twin[key]), key
    assert sorted(envs) == sorted(twin_envs) and rng == twin_rng
    for key in envs:
        assert _same(envs[key], twin_envs[key]), key
    # what the columns say of each other and of the fitness
    table = P.outcome_table_ref(got["rows"])
    steps = table["steps_action0"] + table["steps_action1"] + table["steps_action2"]
    assert np.array_equal(steps, got["env_len"].reshape(n_members, E).sum(axis=1))
    assert _same(steps.astype(np.float64), got["mean_len"] * E)
    assert (table["value_min"] <= got["fitness"]).all() and (got["fitness"] <= table["value_max"]).all()
    return table


@pytest.mark.parametrize("mode", ["greedy", "sample"])
@pytest.mark.parametrize("n_members,E", [(3, 64), (2, 128)])
def test_member_rows_are_the_definition_on_the_recorded_histories_and_nothing_else_changes(n_members, E, mode):
    runs = _rollout_and_its_twin(n_members, E, mode, 0)
    got = runs[0][0]
    w = S.assert_not_vacuous(got["reason"], got["action"])
    assert w["later_ends"] > 0                     # (a dead battery reports itself at every later step: none of those counts)
    table = _assert_rows_and_twin(runs, n_members, E)
    assert table["end_length"].sum() == w["length"] and table["end_wheels"].sum() == w["wheels"]
    assert table["end_battery"].sum() == w["battery"] and table["unfinished"].sum() == w["unfinished"]
    assert len({r.tobytes() for r in got["rows"]}) == n_members        # the members differ


@pytest.mark.parametrize("n_members,E", [(3, 64), (2, 128)])
def test_under_auto_reset_only_the_first_episode_counts(n_members, E):
    runs = _rollout_and_its_twin(n_members, E, "greedy", FLAG_AUTO_RESET)
    got, envs = runs[0][0], runs[0][1]
    w = S.assert_not_vacuous(got["reason"], got["action"])
    table = _assert_rows_and_twin(runs, n_members, E)
    # the envs that ended restarted from the pool and went on: steps and rewards the rows do not count
    n = n_members * E
    assert int(envs["episodes"].sum()) >= 1 and int(envs["episodes"].sum()) == n - w["unfinished"]
    restarted = np.flatnonzero(got["env_len"] < T)
    later = np.array([np.abs(got["reward"][got["env_len"][j]:, j]).sum() for j in restarted])
    assert restarted.size == n - w["unfinished"] and (later != 0).any()
    steps = table["steps_action0"] + table["steps_action1"] + table["steps_action2"]
    assert steps.sum() < T * n and table["unfinished"].sum() == w["unfinished"]


def _world(spec, theta0, n_members, n_val, stream, outcome_capacity):
    total = n_members + n_val
    prop = _propagator(total * 64, FLAG_AUTO_RESET, stream, seed=29, stagger=False, max_length=5)
    pop = P.PolicyPopulation(spec, n_members=total)
    es = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=0.1, lr=0.05, seed=2 ** 33 + 5, log_capacity=4,
                                   validation_members=n_val)
    if outcome_capacity:
        es.set_outcome_log(outcome_capacity)
    return prop, pop, es


def _raw_ring(es):
    C = es.outcome_capacity
    gen, rows = np.empty(C, np.uint64), np.empty((C, 3 * COLS), np.float64)
    _lib.check(es._lib.bsk_es_get_outcome_log(es._handle(), gen.ctypes.data, rows.ctypes.data))
    return gen, rows


def _records(es):
    out = {"theta": es.theta, "generation": np.uint64(es.generation)}
    out.update(("log." + k, v) for k, v in es.training_log().items())
    out.update(("val." + k, v) for k, v in es.validation_log().items())
    out.update(zip(("best.params", "best.fitness", "best.generation", "best.member"), (np.asarray(x) for x in es.best)))
    return out


def test_a_replayed_graph_keeps_the_ring_of_the_eager_loop_and_trains_as_without_it():
    import torch
    from _policy_bounds import seeded_policy
    n_members, n_val, capacity = 4, 2, 2
    spec, theta0 = seeded_policy((16,), "relu", None, seed=33)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        def run(world):
            prop, pop, es = world
            # (episodes of at most 5 steps: every env ends inside the rollout of 8, by LENGTH at the latest)
            es.run_generation(prop, pop, 8, K, "greedy", GAMMA, shared_episodes=True)

        # the eager twin: three generations, the ring rows restated from what each left in device memory
        eager = _world(spec, theta0, n_members, n_val, side.cuda_stream, capacity)
        want_gen = np.full(capacity, P.ES_LOG_EMPTY, np.uint64)
        want_rows = np.zeros((capacity, 3 * COLS))
        empty_gen, empty_rows = _raw_ring(eager[2])
        assert np.array_equal(empty_gen, want_gen) and _same(empty_rows, want_rows)        # the empty start of bsk_es_set_log
        member_rows = []
        for g in range(3):
            run(eager)
            eager[0].sync()
            rows = _download(eager[2].outcomes_ptr(), np.float64, (n_members + n_val) * COLS).reshape(-1, COLS)
            fitness = _download(eager[2].fitness_buffer().ptr, np.float64, n_members + n_val)
            want_gen[g % capacity] = g
            want_rows[g % capacity] = P.es_outcome_row_ref(rows, fitness, n_members, n_val)
            member_rows.append(rows)
        assert _same(_raw_ring(eager[2])[1], want_rows)
        assert not _same(member_rows[1], member_rows[2]) and (member_rows[2][:, :5].sum(axis=1) >= 64).all()
        assert (want_rows[:, 2 * COLS:2 * COLS + 5].sum(axis=1) >= n_val * 64).all()     # block C is no block of zeros
        assert getattr(eager[1], "_outcomes", None) is None
        want = _records(eager[2])

        # the ring off: theta, the training log and the validation log are the same
        plain = _world(spec, theta0, n_members, n_val, side.cuda_stream, 0)
        for g in range(3):
            run(plain)
        plain[0].sync()
        off = _records(plain[2])
        assert sorted(off) == sorted(want)
        for key in want:
            assert _same(off[key], want[key]), key
        with pytest.raises(_lib.BskError):
            plain[2].outcome_log()
        assert plain[2].outcomes_ptr() is None

        # warmed once, two generations captured into one graph, replayed once: three generations, the ring of two wraps
        world = _world(spec, theta0, n_members, n_val, side.cuda_stream, capacity)
        run(world)
        world[0].sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            run(world)
            run(world)
        c0 = BatchedPropagator.debug_counters()
        graph.replay()
        torch.cuda.synchronize()
        assert BatchedPropagator.debug_counters() == c0                  # no copy, no synchronisation across the replayed launches
        gen, rows = _raw_ring(world[2])
        assert np.array_equal(gen, want_gen) and gen.tolist() == [2, 1]
        assert _same(rows, want_rows), (rows, want_rows)
        got = _records(world[2])
        for key in want:
            assert _same(got[key], want[key]), key
        table = world[2].outcome_log()
        assert table["generation"].tolist() == [1, 2]
        assert table["members"]["end_length"].tolist() == [int(want_rows[1, 0]), int(want_rows[0, 0])]
        assert _same(table["best"]["value_max"], np.array([want_rows[1, COLS + 10], want_rows[0, COLS + 10]]))
        for w in (eager, plain, world):
            for x in w:
                x.close()


def test_refusals_come_before_any_launch():
    import torch
    lib = _lib.load()
    n_members, E = 2, 64
    n = n_members * E
    spec, params = S.members(n_members, (16,), seed=91)
    rows = torch.full((n_members + 16, COLS), -7.0, dtype=torch.float64, device="cuda")
    fit = torch.full((n_members,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    pop = P.PolicyPopulation(spec, params)
    es = P.DeviceEvolutionStrategy(spec, params[0], n_members)
    c0 = BatchedPropagator.debug_counters()
    # NULL handles, a negative capacity, a ring without rows, an accessor of a ring that is off
    assert lib.bsk_population_set_outcomes(None, rows.data_ptr()) == -1 and lib.bsk_last_error()
    assert lib.bsk_es_set_outcome_log(None, 1, rows.data_ptr()) == -1
    assert lib.bsk_es_set_outcome_log(es._handle(), -1, rows.data_ptr()) == -1 and b"negative" in lib.bsk_last_error()
    assert lib.bsk_es_set_outcome_log(es._handle(), 2, None) == -1 and b"d_rows" in lib.bsk_last_error()
    assert lib.bsk_es_get_outcome_log(None, None, None) == -1
    assert lib.bsk_es_get_outcome_log(es._handle(), None, None) == -1 and b"bsk_es_set_outcome_log" in lib.bsk_last_error()
    assert BatchedPropagator.debug_counters() == c0
    for bad in (-1, 1.5, True):
        with pytest.raises(ValueError):
            es.set_outcome_log(bad)
    with pytest.raises(ValueError):
        pop.set_outcomes(rows[:n_members].float())
    with pytest.raises(ValueError):
        pop.set_outcomes(rows[:n_members + 1])
    assert es.outcome_capacity == 0 and es.outcomes_ptr() is None
    # a rollout on a handle the population does not fit, with rows attached: refused as ever, nothing written
    odd = _propagator(n + 64, stagger=False)
    pop.set_outcomes(rows[:n_members])
    assert lib.bsk_population_rollout(pop._handle(), odd._handle(), 0, 1, 1, 1.0, *([None] * 8), fit.data_ptr(), None) == -1
    assert lib.bsk_population_rollout(pop._handle(), None, 0, 1, 1, 1.0, *([None] * 8), fit.data_ptr(), None) == -1
    pop.set_outcomes(None)
    odd.close()
    # the first rollout with rows attached allocates their accumulators: refused under capture - the existing rule - even where
    # the population's scratch rows are there already
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        prop = _propagator(n, stream=side.cuda_stream, stagger=False)
        before = _envs(prop)
        pop.rollout_device(prop, 1, 1, d_fitness=fit.data_ptr())
        prop.sync()
        assert bool((fit != -7).all())
        after_one = _envs(prop)
        es.ask(pop, side.cuda_stream)                   # (the optimiser's stream is the one about to be captured)
        prop.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.BskError) as e:
                pop.rollout_device(prop, 1, 1, d_fitness=fit.data_ptr(), d_outcomes=rows.data_ptr())
            assert e.value.code == -1 and "captured" in str(e.value) and "outcome" in str(e.value)
            with pytest.raises(_lib.BskError) as e:     # the ring's setter refuses too, before it allocates or clears anything
                es.set_outcome_log(2)
            assert e.value.code == -1 and "captured" in str(e.value) and es.outcome_capacity == 0
        torch.cuda.synchronize()
        assert getattr(pop, "_outcomes", None) is None
        now = _envs(prop)
        for key in now:
            assert _same(now[key], after_one[key]), key
        assert not _same(before["state"], after_one["state"])
        assert bool((rows == -7).all())
        # ... and the same call outside a capture runs
        pop.rollout_device(prop, 1, 1, d_fitness=fit.data_ptr(), d_outcomes=rows.data_ptr())
        prop.sync()
        assert bool((rows[:n_members] != -7).all()) and bool((rows[n_members:] == -7).all())
        prop.close()
    es.close()
    pop.close()


def test_a_population_and_a_handle_on_different_devices_are_refused():
    if _hip.device_count() < 2:
        pytest.skip("needs two visible devices")
    import torch
    lib = _lib.load()
    spec, params = S.members(2, (16,), seed=91)
    prop = _propagator(128, stagger=False)
    other = P.PolicyPopulation(spec, params, device=1)
    with torch.cuda.device(1):
        rows = torch.full((2, COLS), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
    other.set_outcomes(rows)
    assert lib.bsk_population_rollout(other._handle(), prop._handle(), 0, 1, 1, 1.0, *([None] * 10)) == -1
    assert b"different devices" in lib.bsk_last_error()
    with torch.cuda.device(1):
        torch.cuda.synchronize()
        assert bool((rows == -7).all())
    other.close()
    prop.close()


def test_c_consumer_prints_the_python_bindings_rows(tmp_path):
    """tests/c_abi/c_abi_outcomes.c: bsk_population_set_outcomes and a rollout with no other output from plain C99; its printout
    equals the Python binding's"""
    exe = build_c_consumer(tmp_path, "c_abi_outcomes")
    n_members, E = 3, 64
    n = n_members * E
    ic = sample_ic_batch(n, 4, seed=53)
    spec, params = S.members(n_members, (16,), seed=97)
    ic.tofile(tmp_path / "ic.bin")
    params.tofile(tmp_path / "params.bin")
    got = subprocess.check_output([str(exe), str(tmp_path / "ic.bin"), str(n), str(tmp_path / "params.bin"), str(n_members)]).decode().split()
    assert len(got) == COLS * n_members
    pop = P.PolicyPopulation(spec, params)
    prop = BatchedPropagator(S.config(max_length=4), n)
    prop.reset(ic)
    prop.step(np.zeros(n, np.int32), 5)
    res = pop.evaluate(prop, 6, 5, "greedy", 0.97, outcomes=True)
    want = np.stack([res["outcomes"][name].astype(np.float64) for name in P.OUTCOME_COLUMNS], axis=1)
    assert [float(v) for v in got] == want.ravel().tolist()
    assert res["outcomes"]["end_length"].tolist() == [E] * n_members and res["outcomes"]["unfinished"].tolist() == [0] * n_members
    assert np.array_equal(want[:, 5:8].sum(axis=1), res["env_len"].reshape(n_members, E).sum(axis=1))
    assert len({r.tobytes() for r in want}) == n_members
    prop.close()
    pop.close()
