"""CPU: the numpy restatements of the episode outcomes (policy_ref.py: population_outcomes_ref, es_outcome_row_ref) against a plain
per-env, per-lane Python loop that follows the text of include/bskgpu.h word by word - no vectorisation, no shared helper - on
random histories that hold what the rule can get wrong: a reason byte with two bits set, envs dead at step 0, envs that never
end, NaN values, -0.0, actions outside 0..2.  Every comparison is of bits.  No device and no library is touched.  The last test
runs the scenario of tests/test_gpu_outcomes.py on the CPU oracle, so that what its staggering produces is known before a GPU is.
"""
import math

import numpy as np
import pytest

import _outcome_scenario as S
from _oracle_backend import OraclePropagator
from basilisk_env_amd import policy_ref as R
from basilisk_env_amd._lib import FLAG_AUTO_RESET
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from basilisk_env_amd.policy_spec import OUTCOME_COLS, OUTCOME_COLUMNS, check_outcome_log

NAN = float("nan")


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def _pick(m, x, greatest):
    return x if ((x > m) if greatest else (x < m)) or m != m else m


def _tree_sum(s):
    for stride in (32, 16, 8, 4, 2, 1):
        for l in range(stride):
            s[l] = s[l] + s[l + stride]
    return s[0]


def _tree_pick(m, greatest):
    for stride in (32, 16, 8, 4, 2, 1):
        for l in range(stride):
            m[l] = _pick(m[l], m[l + stride], greatest)
    return m[0]


def _loop_member_rows(reward, reason, action, gamma, E):
    """the definition, one env and one lane at a time, in Python floats (IEEE doubles, every operation rounded on its own)"""
    T, n = reward.shape
    v, end, act_n, length = [0.0] * n, [0] * n, [[0, 0, 0] for _ in range(n)], [0] * n
    for i in range(n):
        g, alive = 1.0, True
        for t in range(T):
            if not alive:
                break
            v[i] = v[i] + g * float(reward[t, i])
            g = g * gamma
            length[i] += 1
            a, q = int(action[t, i]), int(reason[t, i])
            if 0 <= a <= 2:
                act_n[i][a] += 1
            if q != 0:
                end[i], alive = q, False
    rows = []
    for m in range(n // E):
        envs = range(m * E, (m + 1) * E)
        row = [float(sum(1 for i in envs if end[i] & bit)) for bit in (1, 2, 4, 8)]
        row.append(float(sum(1 for i in envs if end[i] == 0)))
        row += [float(sum(act_n[i][k] for i in envs)) for k in range(3)]
        sq, lo, hi = [0.0] * 64, [NAN] * 64, [NAN] * 64
        for l in range(64):
            for c in range(0, E, 64):
                x = v[m * E + l + c]
                sq[l] = x * x if c == 0 else sq[l] + x * x
                lo[l] = x if c == 0 else _pick(lo[l], x, False)
                hi[l] = x if c == 0 else _pick(hi[l], x, True)
        rows.append(row + [_tree_sum(sq), _tree_pick(lo, False), _tree_pick(hi, True)])
    return np.array(rows, np.float64), np.array(length)


def _histories(seed, T, P, E):
    rng = np.random.default_rng(seed)
    n = P * E
    reward = rng.normal(size=(T, n))
    reason = np.where(rng.random((T, n)) < 0.12, rng.choice([1, 2, 4, 8, 3, 5, 6, 12], size=(T, n)), 0).astype(np.uint8)
    action = rng.integers(0, 3, size=(T, n)).astype(np.int32)
    reason[0, 0:n:7] = 2                       # dead at step 0
    reason[0, 5] = 3                           # ... with two bits set
    reason[:, 1:n:5] = 0                       # never ending
    reason[T - 1, 2] = 5                       # ends at the very last step, two bits
    reward[:, 3:n:11] = -0.0                   # a value of zeros of either sign
    reward[1, 4:n:13] = NAN                    # a NaN value (where the env lives to step 1) ...
    reason[:2, 4:n:13] = 0
    reward[:, E:E + 64] = NAN                  # ... and, with P > 1, whole lanes of them
    action[2, 6:n:17] = 7                      # outside 0..2: counted nowhere
    return reward, reason, action


@pytest.mark.parametrize("P,E,gamma", [(3, 64, 0.97), (2, 128, 1.0), (1, 192, 0.5), (2, 320, 0.97), (2, 1024, 1.0)])
def test_member_rows_equal_the_plain_loop(P, E, gamma):
    reward, reason, action = _histories(100 * P + E, 9, P, E)
    got = R.population_outcomes_ref(reward, reason, action, gamma, E)
    want, length = _loop_member_rows(reward, reason, action, gamma, E)
    assert got.shape == (P, OUTCOME_COLS) == (P, len(OUTCOME_COLUMNS))
    assert np.array_equal(_bits(got), _bits(want))
    # the histories hold what they were built to hold
    table = R.outcome_table_ref(got)
    assert table["unfinished"].sum() > 0 and table["end_wheels"].sum() > 0
    assert table["end_length"].sum() + table["end_wheels"].sum() + table["end_battery"].sum() + table["end_orbit"].sum() \
        > P * E - table["unfinished"].sum()                 # some byte counted in two columns
    assert np.isnan(got[0, 8]) and not np.isnan(got[0, 9:]).any()        # a NaN value: in the sum, never an extreme beside a number
    if P > 1:                                                           # ... but the extreme of a member of nothing else
        assert np.isnan(got[1, 9:]).all() == (E == 64)
    # the steps under the three actions are the member's sum of lengths, but for the actions that are none of the three
    fit = R.population_fitness_ref(reward, reason, gamma, P)
    assert np.array_equal(fit["env_len"], length)
    stray = np.array([sum(int(action[t, i]) == 7 for t in range(length[i])) for i in range(P * E)]).reshape(P, E).sum(axis=1)
    assert stray.sum() > 0
    assert np.array_equal(got[:, 5] + got[:, 6] + got[:, 7], fit["env_len"].reshape(P, E).sum(axis=1) - stray)


@pytest.mark.parametrize("E", [64, 192, 320, 1024])
def test_member_rows_carry_non_finite_values_as_the_plain_loop_does(E):
    """What the non-finite runs of tests/test_gpu_population_shapes.py lean on: members whose values hold +inf, -inf, both, a NaN in
    a lane's first element (the incumbent that must be replaced), a NaN in a later one (the candidate that must not win), a NaN
    in front of an infinity - and rewards of -0.0 in a lane's first env, whose value is +0.0 by the rule (v starts from +0.0)"""
    P, T, gamma = 7, 5, 0.97
    rng = np.random.default_rng(E)
    n = P * E
    reward = rng.normal(size=(T, n))
    reason = np.where(rng.random((T, n)) < 0.15, rng.choice([1, 2, 4, 8], size=(T, n)), 0).astype(np.uint8)
    reason[:2] = 0
    action = rng.integers(0, 3, size=(T, n)).astype(np.int32)
    last = E - 1                                                # (with E = 64 every element is a lane's first)
    reward[1, 0 * E + 7] = np.inf
    reward[1, 1 * E + last] = -np.inf
    reward[0, 2 * E + 3], reward[1, 2 * E + last] = np.inf, -np.inf
    reward[1, 3 * E + 5] = NAN                                  # lane 5: a NaN first
    reward[0, 4 * E + last] = NAN                               # lane 63: a NaN last
    reward[0, 5 * E + 9], reward[1, 5 * E + 9] = np.inf, -np.inf                # inf - inf inside one env's value
    reward[0, 5 * E + 10], reward[0, 5 * E + last - 1] = -np.inf, np.inf
    reward[:, 6 * E + 0] = -0.0
    reason[:, 6 * E + 0] = 0
    got = R.population_outcomes_ref(reward, reason, action, gamma, E)
    want, _ = _loop_member_rows(reward, reason, action, gamma, E)
    same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))           # (which NaN a sum makes of inf - inf is the host's)
    assert same.all(), (got[:, 8:], want[:, 8:])
    assert np.array_equal(_bits(got[:, 9:]), _bits(want[:, 9:]))                    # the extremes are picked, not computed: every bit
    assert got[0, 10] == np.inf and got[1, 9] == -np.inf and got[2, 9] == -np.inf and got[2, 10] == np.inf
    assert np.isnan(got[3:6, 8]).all() and not np.isnan(got[:, 9:]).any()
    assert got[5, 9] == -np.inf and got[5, 10] == np.inf
    v = R.population_fitness_ref(reward, reason, gamma, P)["env_value"]
    assert np.isfinite(got[6]).all() and v[6 * E] == 0.0 and not np.signbit(v[6 * E])


def test_steps_by_action_sum_to_the_fitness_lengths():
    P, E = 3, 64
    reward, reason, action = _histories(7, 12, P, E)
    action = np.clip(action, 0, 2)
    rows = R.population_outcomes_ref(reward, reason, action, 0.99, E)
    fit = R.population_fitness_ref(reward, reason, 0.99, P)
    assert np.array_equal(rows[:, 5] + rows[:, 6] + rows[:, 7], fit["env_len"].reshape(P, E).sum(axis=1).astype(np.float64))
    assert np.array_equal(rows[:, 5] + rows[:, 6] + rows[:, 7], fit["mean_len"] * E)
    assert (rows[:, 5:8] > 0).all()


def _loop_totals(rows):
    out = [0.0] * OUTCOME_COLS
    if len(rows) == 0:
        return out
    for c in range(8):
        out[c] = float(sum(int(r[c]) for r in rows))
    sq, lo, hi = [0.0] * 64, [NAN] * 64, [NAN] * 64
    for l in range(64):
        for k in range(l, len(rows), 64):
            sq[l] = float(rows[k][8]) if k == l else sq[l] + float(rows[k][8])
            lo[l] = _pick(lo[l], float(rows[k][9]), False)
            hi[l] = _pick(hi[l], float(rows[k][10]), True)
    out[8], out[9], out[10] = _tree_sum(sq), _tree_pick(lo, False), _tree_pick(hi, True)
    return out


def _beats(a, ia, b, ib):
    na, nb = a != a, b != b
    if na != nb:
        return nb
    if not na and a != b:
        return a > b
    return ia < ib


@pytest.mark.parametrize("P,V", [(2, 0), (6, 2), (70, 1), (130, 16)])
def test_ring_row_equals_the_plain_loop(P, V):
    rng = np.random.default_rng(P + V)
    rows = np.empty((P + V, OUTCOME_COLS))
    rows[:, :8] = rng.integers(0, 5000, size=(P + V, 8))
    rows[:, 8:] = rng.normal(size=(P + V, 3))
    rows[0, 8:] = -0.0                          # -0.0 first and +0.0 behind it: which zero is reported follows from the order
    rows[1, 8:] = 0.0
    rows[P - 1, 9:] = NAN
    if V:
        rows[P, 8:] = NAN
    fitness = rng.normal(size=P + V)
    fitness[0] = NAN
    fitness[P // 2] = fitness[P - 1] = np.nanmax(fitness) + 1.0          # a tie for the first rank: the lower index
    got = R.es_outcome_row_ref(rows, fitness, P, V)
    b = [k for k in range(P) if not any(_beats(fitness[j], j, fitness[k], k) for j in range(P) if j != k)]
    assert b == [P // 2]
    want = _loop_totals(rows[:P]) + list(rows[b[0]]) + _loop_totals(rows[P:])
    assert got.shape == (3 * OUTCOME_COLS,)
    assert np.array_equal(_bits(got), _bits(want))
    if V == 0:
        assert not _bits(got[2 * OUTCOME_COLS:]).any()                  # +0.0, every entry
    # an all-NaN column gives a NaN, and the table names the columns
    rows[:P, 9] = NAN
    assert math.isnan(R.es_outcome_row_ref(rows, fitness, P, V)[9])
    gen = np.array([2 ** 64 - 1, 4, 3], np.uint64)
    table = R.es_outcome_table_ref(gen, np.stack([got * 0, got, got]))
    assert table["generation"].tolist() == [3, 4] and set(table["members"]) == set(OUTCOME_COLUMNS)
    assert table["best"]["end_length"].tolist() == [int(rows[b[0], 0])] * 2 and table["members"]["end_length"].dtype == np.int64


def test_argument_refusals_need_no_device():
    reward, reason, action = _histories(1, 4, 2, 64)
    for bad in (lambda: R.population_outcomes_ref(reward, reason, action[:3], 1.0, 64),
                lambda: R.population_outcomes_ref(reward, reason, action, 1.0, 48),
                lambda: R.population_outcomes_ref(reward, reason, action, 1.0, 0),
                lambda: R.population_outcomes_ref(reward, reason, action, 1.0, 192),
                lambda: R.population_outcomes_ref(reward[0], reason[0], action[0], 1.0, 64),
                lambda: R.es_outcome_row_ref(np.zeros((4, OUTCOME_COLS)), np.zeros(4), 4, 1),
                lambda: R.es_outcome_row_ref(np.zeros((4, OUTCOME_COLS - 1)), np.zeros(4), 4, 0),
                lambda: R.es_outcome_row_ref(np.zeros((4, OUTCOME_COLS)), np.zeros(3), 4, 0),
                lambda: R.es_outcome_row_ref(np.zeros((4, OUTCOME_COLS)), np.zeros(4), 0, 4),
                lambda: R.outcome_table_ref(np.zeros((4, 8))),
                lambda: check_outcome_log(-1), lambda: check_outcome_log(2 ** 31), lambda: check_outcome_log(1.5),
                lambda: check_outcome_log(True), lambda: check_outcome_log(None)):
        with pytest.raises(ValueError):
            bad()
    assert check_outcome_log(0) == 0 and check_outcome_log(np.int32(5)) == 5


@pytest.mark.parametrize("flags", [0, FLAG_AUTO_RESET])
def test_the_staggered_scenario_is_not_vacuous_on_the_oracle(flags):
    """the handle, the staggering and the policies of tests/test_gpu_outcomes.py at (P, E) = (3, 64), greedy, on the oracle backend:
    LENGTH, WHEELS and BATTERY endings spread over the rollout, unfinished envs, all three actions - and rows that say so"""
    P, E, T, k = 3, 64, 12, 1
    n = P * E
    cfg = S.config(flags)
    prop = OraclePropagator(cfg, n)
    if flags:
        prop.set_ic_pool(sample_ic_batch(41, S.N_RW, seed=15))
    prop.reset(sample_ic_batch(n, S.N_RW, seed=14))
    prop.step(np.zeros(n, np.int32), k)
    S.stagger(prop, cfg)
    spec, params = S.members(P, (16,), seed=31, value_hidden=(16,))
    reward, reason, action = S.oracle_histories(prop, spec, params, T, k, E)
    w = S.assert_not_vacuous(reason, action)
    assert w["length"] >= 1 and w["wheels"] >= 1 and w["battery"] >= 1 and w["actions"] == [0, 1, 2]
    assert (w["later_ends"] > 0) == (flags == 0)            # (a dead battery reports itself again at every step, unless it restarts)
    table = R.outcome_table_ref(R.population_outcomes_ref(reward, reason, action, 0.97, E))
    assert table["end_length"].sum() == w["length"] and table["end_wheels"].sum() == w["wheels"]
    assert table["end_battery"].sum() == w["battery"] and table["unfinished"].sum() == w["unfinished"]
    assert (table["value_min"] == -1.0).all()               # (the failure penalty of an env that died at once under an action other than 0)
    if flags:
        assert int(prop.episodes.sum()) == n - w["unfinished"]


def test_the_column_count_is_the_headers():
    import os
    import re
    from basilisk_env_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bskgpu.h")).read()
    (cols,) = re.findall(r"^#define BSK_OUTCOME_COLS (\d+)$", header, re.M)
    assert int(cols) == _lib.BSK_OUTCOME_COLS == OUTCOME_COLS == len(OUTCOME_COLUMNS)
