"""CPU: the numpy restatements of validation on fixed episodes (policy.es_center_ref / es_validate_ref; contract in
include/bskgpu.h, bsk_es_set_validation) held to an operation-by-operation restatement written here with Python's own floats and
struct - one IEEE-754 operation per line, nothing vectorised - on hand cases, and the argument rules of the binding that need no
device.  Every comparison is an equality of bits.  tests/test_gpu_es_validation.py holds the kernels to the same two functions."""
import math
import struct

import numpy as np
import pytest

from basilisk_env_amd import _lib
from basilisk_env_amd import policy as P

NAN, INF = float("nan"), float("inf")
LATE = 2 ** 32 + 3
EMPTY = 2 ** 64 - 1


def _b64(x):
    return struct.unpack("<q", struct.pack("<d", float(x)))[0]


def _b32(x):
    return struct.unpack("<i", struct.pack("<f", x))[0]


def _f32(x):
    """(float)x for a double x, round to nearest even, overflow to inf - through the C conversion numpy's scalar makes"""
    with np.errstate(over="ignore"):
        return float(np.float32(np.float64(x)))


def _step(state, val_f, val_len, generation, theta, C):
    """One tell, operation by operation.  state = [gen list, rows list of 4-lists, params list, best_fitness, best_generation,
    take]; val_f / val_len: the V validation values (val_len None: nothing bound)."""
    gen, rows, params, best, best_gen, _ = state
    V = len(val_f)
    s = val_f[0]
    for v in range(1, V):
        s = s + val_f[v]
    fc = s / float(V)
    if val_len is None:
        lc = 0.0
    else:
        l = val_len[0]
        for v in range(1, V):
            l = l + val_len[v]
        lc = l / float(V)
    take = (not math.isnan(fc)) and (math.isnan(best) or fc > best)
    g = generation % 2 ** 64
    slot = g % C
    gen, rows = list(gen), [list(r) for r in rows]
    rows[slot] = [fc, lc, 1.0 if take else 0.0, float(V)]
    gen[slot] = g
    if take:
        best, best_gen, params = fc, g, [_f32(t) for t in theta]
    return [gen, rows, list(params), best, best_gen, 1 if take else 0]


def _equal(state, ref):
    gen, rows, params, best, best_gen, take = state
    assert [int(x) for x in ref["gen"]] == gen
    assert [[_b64(x) for x in r] for r in ref["rows"]] == [[_b64(x) for x in r] for r in rows]
    assert ref["best_params"].dtype == np.float32 and [_b32(x) for x in ref["best_params"]] == [_b32(x) for x in params]
    assert _b64(ref["best_fitness"]) == _b64(best) or (math.isnan(best) and math.isnan(ref["best_fitness"]))
    assert int(ref["best_generation"]) == best_gen and int(ref["take"]) == take


def test_the_centre_is_the_plain_float_of_every_parameter():
    theta = np.array([-0.0, 0.0, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -40, -1e-50, 1e39, -INF, INF, 0.1, 3.0 * 2.0 ** -150])
    got = P.es_center_ref(theta)
    assert got.dtype == np.float32 and got.shape == theta.shape
    assert [_b32(x) for x in got] == [_b32(_f32(t)) for t in theta]
    # -0.0 stays -0.0 (theta + sigma * 0 would give +0.0); a tie rounds to even, just above it rounds up; 1e39 overflows to +inf
    assert _b32(got[0]) == _b32(-0.0) != _b32(0.0) and _b32(got[4]) == _b32(-0.0)
    assert got[2] == 1.0 and got[3] == np.float32(1.0) + np.float32(2.0 ** -23) and got[5] == INF and got[7] == INF and got[6] == -INF
    assert got[9] == np.float32(2.0 ** -148)               # a denormal: 3 * 2^-150 rounds to 4 * 2^-150
    # not a view of its argument, and a float32 block goes through unchanged
    got[1] = 5.0
    assert theta[1] == 0.0
    block = np.array([0.1, -0.0, 7.0], np.float32)
    assert [_b32(x) for x in P.es_center_ref(block)] == [_b32(x) for x in block]


def test_the_initial_state_is_the_one_of_the_definition():
    st = P.es_validation_state(3, 5, 7, epoch=2 ** 64 - 2)
    assert st["epochs"].dtype == np.uint64 and st["epochs"].tolist() == [2 ** 64 - 2, 2 ** 64 - 1, 0]        # mod 2^64
    assert st["gen"].tolist() == [EMPTY] * 5 and not st["rows"].any() and st["rows"].shape == (5, 4)
    assert st["best_params"].dtype == np.float32 and st["best_params"].shape == (7,) and not st["best_params"].any()
    assert math.isnan(st["best_fitness"]) and st["best_generation"] == EMPTY and st["take"] == 0
    assert P.es_validation_state(1, 1, 1, epoch=0xFFFFFFFF)["epochs"].tolist() == [0xFFFFFFFF]
    for bad in ((0, 4, 7), (17, 4, 7), (1, 0, 7)):
        with pytest.raises(ValueError):
            P.es_validation_state(*bad)


@pytest.mark.parametrize("with_len", [False, True])
@pytest.mark.parametrize("V", [1, 3])
def test_a_sequence_of_tells_by_hand(V, with_len):
    C, P_, n_params = 3, 4, 6
    rng = np.random.default_rng(10 * V + with_len)
    thetas = [rng.normal(size=n_params) for _ in range(9)]
    thetas[0][2] = -0.0
    thetas[5][1] = 1e39
    # the V validation values of each generation; with V = 3 the sums round, and so does the division by 3
    script = {
        1: [[0.5], [NAN], [0.5], [0.25], [0.75], [INF], [INF], [-INF], [NAN]],
        3: [[1.0, 1.0, 2.0 ** 53], [1.0, NAN, 1.0], [2.0 ** 53, 1.0, 1.0], [1.0, 1.0, 2.0 ** 53], [1.0, 1e-17, -1.0], [INF, 1.0, 2.0], [INF, -INF, 0.0],
            [-INF, 0.0, 0.0], [1e308, 1e308, 1e308]],
    }[V]
    ref = P.es_validation_state(V, C, n_params, epoch=7)
    mine = [[EMPTY] * C, [[0.0] * 4 for _ in range(C)], [0.0] * n_params, NAN, EMPTY, 0]
    _equal(mine, ref)
    takes = []
    for r, val in enumerate(script):
        g = LATE + r                                        # (2^32 + 3) mod 3 = 1: the ring wraps in the third tell
        train = rng.normal(size=P_)
        fitness = np.concatenate([train, val])
        lens = np.concatenate([rng.integers(1, 7, size=P_), rng.integers(1, 7, size=V) + rng.integers(0, 8, size=V) / 8.0]).astype(np.float64)
        before = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
        new = P.es_validate_ref(ref, fitness, lens if with_len else None, g, thetas[r])
        for k, v in before.items():                          # the old state is not touched
            assert np.array_equal(v, ref[k], equal_nan=True) if isinstance(v, np.ndarray) else (v == ref[k] or math.isnan(v))
        mine = _step(mine, [float(x) for x in val], [float(x) for x in lens[P_:]] if with_len else None, g, [float(t) for t in thetas[r]], C)
        _equal(mine, new)
        # the training members' values are never read: other ones give the same state
        other = P.es_validate_ref(ref, np.concatenate([train[::-1] * 3.0, val]), lens if with_len else None, g, thetas[r])
        _equal(mine, other)
        # ... and the V values alone are the last V values of themselves
        _equal(mine, P.es_validate_ref(ref, np.array(val), lens[P_:] if with_len else None, g, thetas[r]))
        takes.append(new["take"])
        ref = new
    if V == 1:
        # take; NaN never takes; the tie keeps the older champion; lower; higher; +inf; +inf ties +inf; -inf; NaN
        assert takes == [1, 0, 0, 0, 1, 1, 0, 0, 0]
        assert ref["best_generation"] == LATE + 5 and ref["best_fitness"] == INF
        assert [_b32(x) for x in ref["best_params"]] == [_b32(_f32(t)) for t in thetas[5]] and ref["best_params"][1] == INF
    else:
        # (1 + 1) + 2^53 = 2^53 + 2 but (2^53 + 1) + 1 = 2^53: the order of the sum is the definition's, ascending from f[P] - the
        # same three values in the other order score lower and do not take; the first order again ties and does not take either
        assert (1.0 + 1.0) + 2.0 ** 53 == 2.0 ** 53 + 2.0 and (2.0 ** 53 + 1.0) + 1.0 == 2.0 ** 53
        assert takes == [1, 0, 0, 0, 0, 1, 0, 0, 0]
        assert ref["best_generation"] == LATE + 5 and ref["best_fitness"] == INF
        # (inf - inf) / 3 is a NaN and 3e308 overflows to +inf, which ties the champion: neither takes
        assert math.isnan(ref["rows"][(LATE + 6) % C][0]) and ref["rows"][(LATE + 8) % C][0] == INF
    # the ring of three holds the last three generations, each in the slot of its whole 64-bit word
    assert sorted(int(x) for x in ref["gen"]) == [LATE + 6, LATE + 7, LATE + 8]
    for slot in range(C):
        assert int(ref["gen"][slot]) % C == slot and ref["rows"][slot][3] == float(V)
    assert (LATE % C, 3 % C) == (1, 0)                       # the low word alone would fall into another slot
    table = P.es_validation_table_ref(ref["gen"], ref["rows"])
    assert table["generation"].tolist() == [LATE + 6, LATE + 7, LATE + 8] and table["members"].tolist() == [V] * 3
    assert table["take"].dtype == np.int64 and table["take"].tolist() == takes[6:]
    assert [_b64(x) for x in table["fitness"]] == [_b64(ref["rows"][(LATE + r) % C][0]) for r in (6, 7, 8)]
    assert sorted(table) == sorted(("generation",) + P.ES_VAL_COLUMNS)
    if not with_len:
        assert all(_b64(x) == _b64(0.0) for x in table["mean_len"])


def test_the_first_champion_of_a_tie_is_the_older_one():
    ref = P.es_validation_state(1, 2, 3)
    ref = P.es_validate_ref(ref, [9.0, 9.0, 2.0], None, 0, [1.0, 2.0, 3.0])
    again = P.es_validate_ref(ref, [0.0, 0.0, 2.0], None, 1, [4.0, 5.0, 6.0])
    assert ref["take"] == 1 and again["take"] == 0 and again["best_generation"] == 0 and again["best_params"].tolist() == [1.0, 2.0, 3.0]
    assert again["rows"][1].tolist() == [2.0, 0.0, 0.0, 1.0] and again["rows"][0].tolist() == [2.0, 0.0, 1.0, 1.0]
    # -0.0 against +0.0 is a tie as well
    z = P.es_validate_ref(P.es_validation_state(1, 2, 3), [-0.0], None, 0, [0.0] * 3)
    assert z["take"] == 1 and P.es_validate_ref(z, [0.0], None, 1, [1.0] * 3)["take"] == 0
    with pytest.raises(ValueError):
        P.es_validate_ref(P.es_validation_state(3, 2, 3), [1.0, 2.0], None, 0, [0.0] * 3)
    with pytest.raises(ValueError):
        P.es_validate_ref(ref, [1.0, 2.0], [1.0], 0, [0.0] * 3)


def test_the_argument_rules_that_need_no_device():
    assert P.check_validation(0) == (0, 64, 0)
    assert P.check_validation(1, None, 0xFFFFFFFF, 12) == (1, 12, 0xFFFFFFFF)
    assert P.check_validation(16, 5, 2 ** 64 - 17) == (16, 5, 2 ** 64 - 17)
    assert P.check_validation(np.int64(3), np.int32(2), np.uint64(9)) == (3, 2, 9)
    assert P.check_validation(0, 0) == (0, 0, 0)            # (off: the capacity is not looked at, as bsk_es_set_validation does not)
    for bad in ((-1,), (17,), (1.5,), (True,), (1, 0), (1, -2), (1, 2 ** 31), (1, 2.5), (1, 4, -1), (1, 4, 2 ** 64 - 16), (1, 4, 0.5)):
        with pytest.raises(ValueError):
            P.check_validation(*bad)
    assert P.ES_VAL_MAX_MEMBERS == 16 and P.ES_VAL_COLUMNS == ("fitness", "mean_len", "take", "members")
    # the constructor refuses before it touches the library
    spec = P.check_spec((16,), "relu")
    for kw in (dict(validation_members=17), dict(validation_members=-1), dict(validation_members=1, validation_capacity=0),
               dict(validation_members=2, validation_epoch=-5), dict(validation_members=1.5)):
        with pytest.raises(ValueError):
            P.DeviceEvolutionStrategy(spec, None, 4, **kw)
    # the exports and their signatures are declared, and the new names are the module's
    for name in ("bsk_es_set_validation", "bsk_es_get_validation_log", "bsk_es_get_validated_best", "bsk_es_set_validated_best",
                 "bsk_es_validated_best_device", "bsk_es_validation_epochs_device", "bsk_population_set_obs_stats_members"):
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["bsk_es_set_validation"][0]) == 5
    for name in ("set_validation", "validation_log", "validated_best", "set_validated_best", "validated_best_params_ptr", "members_total"):
        assert hasattr(P.DeviceEvolutionStrategy, name)
    assert hasattr(P.PolicyPopulation, "set_obs_stats_members")
