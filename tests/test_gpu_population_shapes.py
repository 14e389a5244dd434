"""GPU: the population path of a generation at many members and many waves per member (bsk_population_act / _rollout,
bsk_population_set_outcomes, bsk_es_set_outcome_log; policy_population_kernel in csrc/bsk_policy.hip, fitness_join_kernel and
outcome_join_kernel in csrc/bsk_population.hip, es_outcome_kernel in csrc/bsk_es.hip; contract in include/bskgpu.h).

tests/test_gpu_population.py and tests/test_gpu_outcomes.py hold these kernels to their definitions at E = 64 and 128 and at most
five members: one or two policy workgroups per member, at most two trips of the join kernels' lane loop, one join workgroup, four
members in the 64 lanes of the evolution strategy's records.  The shapes here (tests/_population_cases.py) are the smallest past
each of those: three, five and sixteen trips and workgroups per member, up to nine join workgroups with a partial last one, and 130
members for the records.  Every check is an EQUALITY of bits - against one policy launch or one policy rollout per member, against
bsk_select_branches, and against the numpy restatements (population_fitness_ref, population_outcomes_ref, es_outcome_row_ref,
es_log_row_ref, es_validate_ref, which tests/test_population_host.py, test_outcomes_host.py, test_es_log_host.py and
test_es_validation_host.py hold to plain loops at these shapes).  One exception the arithmetic makes itself, in the non-finite runs
only: which NaN a sum or a product makes of +inf and -inf, and which of two NaN operands it hands on, is not defined, so a value
that went through an addition compares there as "the same bits, or a NaN in both".

That a reordered sum would be seen is a condition every rollout test of cases a, b and c asserts on its own data
(_population_cases.assert_order_is_visible); tests/test_population_host.py proves it beforehand on the CPU oracle.
"""
import ctypes

import numpy as np
import pytest

import _population_cases as C
from _device_bits import download as _download, same as _same
from _policy_bounds import observation_like, seeded_policy
from basilisk_env_amd import _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET
from basilisk_env_amd.simulators.dynamics import BatchedPropagator

pytestmark = pytest.mark.gpu

COLS = P.OUTCOME_COLS
T, K, GAMMA = C.T, C.K, C.GAMMA


# ---------------------------------------------------------------------------------------------------------------------------------
# bsk_population_act

# [16] alone; [32, 16] beside a narrower value network; [16] beside a WIDER one, so that the launch's LDS width comes from the value side
SPECS = {"plain": ((16,), None), "value": ((32, 16), (16,)), "wide_value": ((16,), (48, 32))}


def _act_members(n_members, hidden, activation, value_hidden, seed):
    blocks = []
    for m in range(n_members):
        spec, block = seeded_policy(hidden, activation, value_hidden, seed=seed + 17 * m)
        blocks.append(block)
    params = np.stack(blocks)
    assert len({b.tobytes() for b in params}) == n_members
    return spec, params


@pytest.mark.parametrize("activation", ["relu", "tanh"])
@pytest.mark.parametrize("spec_name", sorted(SPECS))
@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_act_equals_one_policy_launch_per_member_and_the_numpy_chain(case, spec_name, activation):
    import torch
    lib = _lib.load()
    n_members, E = C.SHAPES[case]
    hidden, value_hidden = SPECS[spec_name]
    n, pad = n_members * E, 37
    spec, params = _act_members(n_members, hidden, activation, value_hidden, seed=3)
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

    def launch(d_obs, out, mode, base):
        _lib.check(lib.bsk_population_act(pop._handle(), d_obs.data_ptr(), n + pad, n, E, base, mode, out["action"].data_ptr(),
                                          out["logp"].data_ptr(), out["value"].data_ptr() if value_hidden is not None else None,
                                          out["logits"].data_ptr(), n + 64, None))
    # greedy from a small env_base, sample from one past 2^32: the draw is keyed by all 64 bits of env_base + j
    for mode, base in ((0, 1000), (1, 2 ** 40 + 1000)):
        got, want = outputs(), outputs()
        pop.set_rng(9, 5)
        for pol in singles:
            pol.set_rng(9, 5)
        torch.cuda.synchronize()
        launch(block, got, mode, base)
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
            assert _same(got[key], want[key]), (mode, key, np.flatnonzero((got[key] != want[key]).reshape(-1, n + 64).any(axis=0))[:8] // E)
        assert (got["action"][n:] == -7).all() and (got["logits"][:, n:] == -7).all() and (got["logp"][n:] == -7).all()
        assert got["action"][:n].min() >= 0 and got["action"][:n].max() <= 2 and (got["logp"][:n] != -7).all()
        assert (got["value"][:n] != -7).all() if value_hidden is not None else (got["value"] == -7).all()
        # the draw counter: one more per population launch that sampled, as after one launch of a single policy
        assert pop.get_rng() == singles[0].get_rng() == (9, 5 + mode)
        if mode == 1:
            assert len(set(got["action"][:n].tolist())) > 1
            launch(block, outputs(), mode, base)
            assert pop.get_rng() == (9, 7)
        if activation == "relu" and mode == 0:
            for m in range(n_members):       # the definition itself, member by member: a wrong block offset cannot pass
                cols = slice(m * E, (m + 1) * E)
                l, v = P.mlp_ref(spec, params[m], obs[:, cols])
                assert _same(got["logits"][:, cols], l) and np.array_equal(got["action"][cols], P.act_ref(l, "greedy")[0]), m
                if value_hidden is not None:
                    assert _same(got["value"][cols], v), m
    assert bool(torch.isnan(block[:, n:]).all())
    # a wrong block would be seen: on the SAME E observations no two members give the same logits (nor the same values)
    tiled = torch.full((5, n + pad), float("nan"), dtype=torch.float64, device="cuda")
    tiled[:, :n] = torch.from_numpy(np.tile(obs[:, :E], (1, n_members))).cuda()
    out = outputs()
    torch.cuda.synchronize()
    launch(tiled, out, 0, 0)
    torch.cuda.synchronize()
    logits = out["logits"].cpu().numpy()[:, :n].reshape(3, n_members, E)
    assert len({logits[:, m].tobytes() for m in range(n_members)}) == n_members
    assert len({logits[k, m].tobytes() for m in range(n_members) for k in range(3)}) == 3 * n_members
    if value_hidden is not None:
        value = out["value"].cpu().numpy()[:n].reshape(n_members, E)
        assert len({value[m].tobytes() for m in range(n_members)}) == n_members
    for x in singles + [pop]:
        x.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# bsk_population_rollout: fitness and outcome rows

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


def _member_slice(key, val, m, E):
    """member m's part of one of _envs' arrays of the whole handle"""
    if key == "done_mask":
        return val[m * E // 64:(m + 1) * E // 64]
    return val[..., m * E:(m + 1) * E]


def _buffers(n, n_members):
    import torch
    bufs = {key: torch.zeros(T * n * size, dtype=torch.uint8, device="cuda") for key, size, _, _ in C.HIST}
    bufs["env_value"] = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    bufs["env_len"] = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    bufs["fitness"] = torch.full((n_members,), -7.0, dtype=torch.float64, device="cuda")
    bufs["mean_len"] = torch.full((n_members,), -7.0, dtype=torch.float64, device="cuda")
    bufs["rows"] = torch.full((n_members, COLS), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return bufs


def _host(bufs, n):
    out = {key: bufs[key].cpu().numpy().view(dt).reshape((T, 5, n) if rows == 5 else (T, n)) for key, _, dt, rows in C.HIST}
    for key in ("env_value", "env_len", "fitness", "mean_len", "rows"):
        out[key] = bufs[key].cpu().numpy()
    return out


RNG = C.SAMPLE_RNG


def _rollout_and_its_twin(case, mode, cfg, select=False):
    """One rollout of the case's scenario with outcome rows and all six histories, and the same rollout on a twin handle and a twin
    population that never heard of outcomes -> [(host results, handle buffers, draw counter)] of each; with ``select`` the first
    also holds bsk_select_branches' values of the histories it recorded, one group per member"""
    import torch
    n_members, E = C.SHAPES[case]
    n = n_members * E
    spec, params = C.members(case)
    ic = C.initial_conditions(n, C.IC_SEED[case])
    runs = []
    for outcomes in (True, False):
        prop = C.staged(BatchedPropagator, cfg, ic)
        pop = P.PolicyPopulation(spec, params)
        pop.set_rng(*RNG)
        bufs = _buffers(n, n_members)
        pop.rollout_device(prop, T, K, mode, GAMMA, *(bufs[key].data_ptr() for key, _, _, _ in C.HIST),
                           d_env_value=bufs["env_value"].data_ptr(), d_env_len=bufs["env_len"].data_ptr(),
                           d_fitness=bufs["fitness"].data_ptr(), d_mean_len=bufs["mean_len"].data_ptr(),
                           d_outcomes=bufs["rows"].data_ptr() if outcomes else None)
        if select and outcomes:
            first = torch.zeros(n, dtype=torch.int32, device="cuda")
            values = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
            best = torch.zeros(n_members, dtype=torch.int32, device="cuda")
            prop.sync()
            _lib.check(_lib.load().bsk_select_branches(bufs["reward"].data_ptr(), bufs["reason"].data_ptr(), first.data_ptr(), T, n, E,
                                                       GAMMA, values.data_ptr(), None, best.data_ptr(),
                                                       ctypes.c_void_p(prop.stream_ptr())))
        prop.sync()
        assert getattr(pop, "_outcomes", None) is None          # attached for the call only
        host = _host(bufs, n)
        if select and outcomes:
            host["select_values"] = values.cpu().numpy()
        runs.append((host, _envs(prop), pop.get_rng()))
        prop.close()
        pop.close()
    return runs, (spec, params, ic)


def _assert_twin(runs):
    """without outcomes every other output and the handle are the same, bit for bit, and no row is written"""
    (got, envs, rng), (twin, twin_envs, twin_rng) = runs
    assert (twin["rows"] == -7.0).all() and (got["rows"] != -7.0).all()
    for key in twin:
        if key != "rows":
            assert _same(got[key], twin[key]), key
    assert sorted(envs) == sorted(twin_envs) and rng == twin_rng
    for key in envs:
        assert _same(envs[key], twin_envs[key]), key


SEPARATE = {"a": range(7), "b": (0, 8), "c": (0, 5), "d": (0, 16, 32)}


@pytest.mark.parametrize("mode", ["greedy", "sample"])
@pytest.mark.parametrize("case", ["a", "b", "c", "d"])
def test_rollout_is_its_definitions_and_the_separate_rollouts(case, mode):
    n_members, E = C.SHAPES[case]
    n = n_members * E
    cfg = C.config(FLAG_AUTO_RESET)
    runs, (spec, params, ic) = _rollout_and_its_twin(case, mode, cfg, select=True)
    got, envs, rng = runs[0]
    assert rng == (RNG[0], RNG[1] + (T if mode == "sample" else 0))
    # (1) the definitions on the recorded histories
    ref = P.population_fitness_ref(got["reward"], got["reason"], GAMMA, n_members)
    for key in ("env_value", "env_len", "fitness", "mean_len"):
        assert _same(got[key], ref[key]), (key, np.flatnonzero(got[key] != ref[key])[:8])
    rows = P.population_outcomes_ref(got["reward"], got["reason"], got["action"], GAMMA, E)
    for c in range(COLS):
        assert _same(got["rows"][:, c], rows[:, c]), (c, got["rows"][:, c], rows[:, c])
    assert _same(got["env_value"], got["select_values"])
    table = P.outcome_table_ref(got["rows"])
    steps = table["steps_action0"] + table["steps_action1"] + table["steps_action2"]
    assert np.array_equal(steps, got["env_len"].reshape(n_members, E).sum(axis=1))
    assert (table["value_min"] <= got["fitness"]).all() and (got["fitness"] <= table["value_max"]).all()
    assert len({r.tobytes() for r in got["rows"]}) == n_members        # the members differ
    # (2) the scenario did not come out empty: every member has LENGTH and WHEELS endings at staggered steps, unfinished envs, values
    # of both signs; the envs that ended restarted and went on earning reward that does not count
    w = C.assert_every_member_is_mixed(got["reward"], got["reason"], got["action"], E)
    restarted = np.flatnonzero(got["env_len"] < T)
    later = np.array([np.abs(got["reward"][got["env_len"][j]:, j]).sum() for j in restarted])
    assert int(envs["episodes"].sum()) >= restarted.size > 0 and (later != 0).any()
    full = P.population_fitness_ref(got["reward"], np.zeros_like(got["reason"]), GAMMA, n_members)
    assert not np.array_equal(full["fitness"], got["fitness"])
    print(case, mode, {k: (int(v.min()), int(v.max())) for k, v in w.items()})
    # (3) ... and the order of the join's additions shows: with more than one trip, the trips added in descending order or into two
    # alternating accumulators give other bits than the definition, in the fitness and in the sum of squares
    if E > 64:
        print(case, mode, C.order_is_visible(got["env_value"], E)[0])
        C.assert_order_is_visible(got["env_value"], E, got["fitness"], got["rows"][:, 8])
    # (4) outcomes off: nothing else changes
    _assert_twin(runs)
    # (5) the same histories and the same handle as separate rollouts of single policies on handles of E envs
    for m in SEPARATE[case]:
        cols = slice(m * E, (m + 1) * E)
        part = C.staged(BatchedPropagator, cfg, ic[:, cols], first=m * E)
        pol = P.DevicePolicy(spec, params[m])
        pol.set_rng(*RNG)
        want = pol.rollout(part, T, K, mode)
        for key in ("obs", "reward", "reason", "action", "logp", "value"):
            assert _same(got[key][..., cols], want[key]), (m, key)
        eb = _envs(part)
        assert set(envs) == set(eb) and "episodes" in envs
        for key in envs:
            assert _same(_member_slice(key, envs[key], m, E), eb[key]), (m, key)
        part.close()
        pol.close()
    assert len(set(got["action"].ravel().tolist())) == 3


@pytest.mark.parametrize("reward_mult", [C.REWARD_MULT, C.INF], ids=["penalty_inf", "penalty_and_reward_inf"])
def test_non_finite_values_go_through_the_joins_by_their_rules(reward_mult):
    """failure_penalty = +inf: an env that fails holds -inf.  With reward_mult = +inf too, a step under action 0 earns +inf, a step
    that fails under it inf - inf, and a member holds NaN, -inf and +inf among its numbers: in a lane's first trip (where the join
    starts from the value) and in a later one (where it is a candidate against the incumbent)"""
    case = "n"
    n_members, E = C.SHAPES[case]
    cfg = C.config(FLAG_AUTO_RESET, reward_mult, C.INF)
    runs, _ = _rollout_and_its_twin(case, "greedy", cfg)
    got = runs[0][0]
    v = got["env_value"]
    first_trip, later_trip = C.nan_positions(v, E)
    print("nan in first trip / later trip (members):", first_trip, later_trip, "-inf", int(np.isneginf(v).sum()), "+inf",
          int(np.isposinf(v).sum()), "nan", int(np.isnan(v).sum()), "finite", int(np.isfinite(v).sum()))
    by_member = v.reshape(n_members, E)
    if reward_mult == C.INF:
        assert first_trip >= 1 and later_trip >= 1
        assert not np.isnan(by_member).all(axis=1).any()
        assert np.isposinf(v).any() and np.isneginf(v).any() and np.isfinite(v).any()
        # a lane whose FIRST value is a NaN and which sees a number later: the incumbent that has to be replaced
        lanes = by_member.reshape(n_members, E // 64, 64)
        assert (np.isnan(lanes[:, 0]) & ~np.isnan(lanes[:, 1:]).all(axis=1)).any()
        assert (~np.isnan(lanes[:, 0]) & np.isnan(lanes[:, 1:]).any(axis=1)).any()
    else:
        assert not np.isnan(v).any() and (np.isneginf(by_member).any(axis=1) & np.isfinite(by_member).any(axis=1)).all()
    ref = P.population_fitness_ref(got["reward"], got["reason"], GAMMA, n_members)
    rows = P.population_outcomes_ref(got["reward"], got["reason"], got["action"], GAMMA, E)
    assert _same(got["env_len"], ref["env_len"]) and _same(got["mean_len"], ref["mean_len"])
    for key in ("env_value", "fitness"):
        assert C.same_or_nan(got[key], ref[key]), (key, got[key], ref[key])
    assert _same(got["rows"][:, :8], rows[:, :8])
    assert C.same_or_nan(got["rows"][:, 8], rows[:, 8]), (got["rows"][:, 8], rows[:, 8])
    # the extremes are picked, not computed: a NaN incumbent is replaced, a NaN candidate never wins - every bit is defined
    assert _same(got["rows"][:, 9:], rows[:, 9:]), (got["rows"][:, 9:], rows[:, 9:])
    assert not np.isnan(got["rows"][:, 9:]).any() and np.isneginf(got["rows"][:, 9]).sum() >= n_members - 1
    with np.errstate(invalid="ignore"):
        assert _same(got["rows"][:, 9], np.nanmin(by_member, axis=1)) and _same(got["rows"][:, 10], np.nanmax(by_member, axis=1))
    assert not np.isfinite(got["fitness"]).any() and not np.isfinite(got["rows"][:, 8]).any()
    _assert_twin(runs)


# ---------------------------------------------------------------------------------------------------------------------------------
# the evolution strategy's records at more members than lanes

def _raw(es, name, capacity, width):
    gen, rows = np.empty(capacity, np.uint64), np.empty((capacity, width), np.float64)
    _lib.check(getattr(es._lib, "bsk_es_get_" + name)(es._handle(), gen.ctypes.data, rows.ctypes.data))
    return gen, rows


@pytest.mark.parametrize("reward_mult,failure_penalty", [(C.REWARD_MULT, C.FAILURE_PENALTY), (C.INF, C.INF)], ids=["finite", "non_finite"])
def test_the_generation_records_at_130_members_are_their_restatements(reward_mult, failure_penalty):
    """P = 130 ranked members and V = 3 validation members of 64 envs: block A of the outcome ring walks three trips of the 64 lanes
    (130 = 64 + 64 + 2), block C three lanes, and block B is the row of a champion a later trip holds"""
    n_members, E = C.SHAPES["e"]
    n_val, capacity, n_gen = C.ES["n_val"], 4, 2
    total = n_members + n_val
    finite = reward_mult != C.INF
    same = _same if finite else C.same_or_nan
    spec, theta0 = C.es_start()
    cfg = C.config(FLAG_AUTO_RESET, reward_mult, failure_penalty, max_length=C.ES["max_length"])
    prop = C.es_handle(BatchedPropagator, cfg, total * E)
    pop = P.PolicyPopulation(spec, n_members=total)
    pop.set_rng(*C.ES["rng"])
    es = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=C.ES["sigma"], lr=C.ES["lr"], seed=C.ES["seed"], log_capacity=capacity,
                                   validation_members=n_val)
    es.set_outcome_log(capacity)
    val = P.es_validation_state(n_val, capacity, P.n_params(spec), es.validation_epoch)
    want_gen = np.full(capacity, P.ES_LOG_EMPTY, np.uint64)
    want_ring, want_log = np.zeros((capacity, 3 * COLS)), np.zeros((capacity, 8))
    champions = []
    for g in range(n_gen):
        theta = es.theta
        es.run_generation(prop, pop, C.ES["T"], K, C.ES["mode"], GAMMA, shared_episodes=True)
        prop.sync()
        rows = _download(es.outcomes_ptr(), np.float64, total * COLS).reshape(total, COLS)
        fitness = _download(es.fitness_buffer().ptr, np.float64, total)
        mean_len = _download(es._out["mean_len"].ptr, np.float64, total)
        assert np.isfinite(fitness).all() if finite else np.isnan(fitness[:n_members]).any()
        if finite:                                                      # the member rows are pairwise distinct: block B is one row only
            assert len({r.tobytes() for r in rows}) == total
        assert (rows[:, :5].sum(axis=1) >= E).all() and (mean_len >= 1.0).all() and (mean_len <= C.ES["T"]).all()
        # the champion under the order of the ranking, in plain Python: a number beats a NaN, the greater number wins, a tie goes
        # to the lower index
        b = 0
        for k in range(1, n_members):
            fk, fb = float(fitness[k]), float(fitness[b])
            if (fb != fb and fk == fk) or fk > fb:
                b = k
        champions.append(b)
        want_gen[g] = g
        want_ring[g] = P.es_outcome_row_ref(rows, fitness, n_members, n_val)
        assert _same(want_ring[g, COLS:2 * COLS], rows[b])
        want_log[g] = P.es_log_row_ref(fitness[:n_members], mean_len[:n_members])
        val = P.es_validate_ref(val, fitness, mean_len, g, theta)
        gen, ring = _raw(es, "outcome_log", capacity, 3 * COLS)
        assert np.array_equal(gen, want_gen) and same(ring, want_ring), (g, ring[g], want_ring[g])
        assert _same(ring[g, COLS:2 * COLS], rows[b]) and _same(ring[g, :8], rows[:n_members, :8].sum(axis=0))
        assert _same(ring[g, 2 * COLS:2 * COLS + 8], rows[n_members:, :8].sum(axis=0))
        gen, log = _raw(es, "log", capacity, 8)
        assert np.array_equal(gen, want_gen) and same(log, want_log), (g, log[g], want_log[g])
        assert int(log[g, 5]) == b
        gen, rows_val = _raw(es, "validation_log", capacity, 4)
        assert np.array_equal(gen, val["gen"]) and same(rows_val, val["rows"]), (g, rows_val[g], val["rows"][g])
        assert es.generation == g + 1
    print("champions:", champions)
    if finite:
        # block B came from a later trip of the 64 lanes in at least one generation (tests/test_population_host.py finds the first
        # generation's champion on the CPU oracle)
        assert max(champions) >= 64, champions
    table = es.outcome_log()
    assert table["generation"].tolist() == list(range(n_gen))
    assert table["members"]["end_length"].tolist() == [int(want_ring[g, 0]) for g in range(n_gen)]
    for x in (prop, pop, es):
        x.close()
