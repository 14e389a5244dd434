"""CPU: planning with a learned value at the leaves - the numpy statements of bsk_select_branches_boot and bsk_beam_select_boot
(planning.branch_values_boot / beam_select_boot_ref; the GPU tests hold the kernels to them bit for bit), the refusals of the three
C entry points, which need no device, and the planners' argument rules."""
import types

import numpy as np
import pytest

from basilisk_env_amd import _lib, planning
from basilisk_env_amd.policy_spec import check_spec


def _histories(rng, T, nb):
    r = rng.normal(size=(T, nb)) * 1e-2
    r[:, ::4] = np.round(r[:, ::4], 3)
    q = ((rng.random((T, nb)) < 0.15) * rng.integers(1, 16, (T, nb))).astype(np.uint8)
    q[:, 0] = 0                                         # a branch that never ends
    q[0, 1] = 3                                         # an end at step 0
    q[:, 2] = 0
    q[T - 1, 2] = 1                                     # an end at the last step, and only there: no bootstrap
    leaf = rng.normal(size=nb).astype(np.float32)
    leaf[3:8] = [np.nan, np.inf, -np.inf, -0.0, 0.0]
    q[:, 3:8] = 0                                       # (the special leaves all count)
    return r, q, leaf


def _brute_force(r, q, gamma, leaf):
    """the definition of include/bskgpu.h, one branch at a time in Python floats (IEEE doubles, one rounding per operation)"""
    T, nb = r.shape
    out = np.empty(nb)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(nb):
            v, g, ended = np.float64(0.0), np.float64(1.0), False
            for t in range(T):
                p = g * np.float64(r[t, b])
                v = v + p
                g = g * np.float64(gamma)
                if q[t, b] != 0:
                    ended = True
                    break
            if not ended:
                p = g * np.float64(np.float32(leaf[b]))
                v = v + p
            out[b] = v
    return out


@pytest.mark.parametrize("gamma", [1.0, 0.99, 0.0])
@pytest.mark.parametrize("T", [1, 2, 5])
def test_branch_values_boot_is_the_definition_branch_by_branch(gamma, T):
    rng = np.random.default_rng(100 * T + int(10 * gamma))
    r, q, leaf = _histories(rng, T, 60)
    got = planning.branch_values_boot(r, q, gamma, leaf)
    want = _brute_force(r, q, gamma, leaf)
    assert got.tobytes() == want.tobytes()              # bit for bit, NaN payloads and the sign of zero included
    plain = planning.branch_values(r, q, gamma)
    assert got[1] == plain[1] and got[2] == plain[2]    # ended at step 0 / at the last step: no leaf term
    if T > 1:
        assert q[0, 1] != 0 and (q[:T - 1, 2] == 0).all() and q[T - 1, 2] != 0
    assert np.isnan(got[3])                             # a NaN leaf makes the branch NaN ...
    if gamma != 0.0:
        assert got[4] == np.inf and got[5] == -np.inf
    best, _ = planning.select_best(got[:6], 6)
    assert best != 3                                    # ... and a NaN loses


@pytest.mark.parametrize("gamma", [1.0, 0.99])
def test_a_zero_leaf_changes_nothing(gamma):
    rng = np.random.default_rng(7)
    r, q, _ = _histories(rng, 4, 90)
    assert np.array_equal(planning.branch_values_boot(r, q, gamma, np.zeros(90, np.float32)), planning.branch_values(r, q, gamma))


def _level(rng, n_roots, width):
    n = 3 * width * n_roots
    r = np.round(rng.normal(size=n) * 1e-2, 3)
    q = ((rng.random(n) < 0.2) * rng.integers(1, 16, n)).astype(np.uint8)
    slots = np.zeros(n_roots * width, dtype=planning.BEAM_SLOT)
    slots["value"] = np.round(rng.normal(size=len(slots)), 2)
    slots["first"] = rng.integers(0, 3, len(slots))
    slots["flags"] = rng.choice([0, planning.BEAM_VALID, planning.BEAM_VALID | planning.BEAM_LIVE], len(slots), p=[0.1, 0.2, 0.7])
    return r, q, slots


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("width", [1, 3, 9])
def test_beam_boot_with_a_zero_leaf_is_beam_select(level, width):
    rng = np.random.default_rng(width + level)
    n_roots = 7
    r, q, slots = _level(rng, n_roots, width)
    zero = np.zeros(3 * width * n_roots, np.float32)
    out, fmap, keys, best_value, best_action = planning.beam_select_boot_ref(r, q, zero, n_roots, width, level, 0.97, 0.95, slots)
    want = planning.beam_select_ref(r, q, n_roots, width, level, 0.97, slots)
    assert out.tobytes() == want[0].tobytes()
    assert np.array_equal(fmap, want[1]) and np.array_equal(best_action, want[3])
    assert np.array_equal(keys, out["value"], equal_nan=True) and np.array_equal(best_value, want[2], equal_nan=True)


def test_beam_boot_ranks_by_the_key_and_keeps_the_value():
    """One root, width 2, level 0: rewards 3 > 2 > 1 for actions 0, 1, 2, action 0's episode ends.  The leaf lifts action 2 over
    action 1 and cannot lift the ended action 0: by value the kept pair is (0, 1), by key it is (2, 0)."""
    r = np.zeros(6)
    r[:3] = [3.0, 2.0, 1.0]
    q = np.zeros(6, np.uint8)
    q[0] = 1
    leaf = np.array([100.0, 0.5, 6.0, 0.0, 0.0, 0.0], np.float32)
    plain = planning.beam_select_ref(r, q, 1, 2, 0, 1.0)
    out, fmap, keys, best_value, best_action = planning.beam_select_boot_ref(r, q, leaf, 1, 2, 0, 1.0, 0.5)
    assert list(plain[1]) == [0, 1] and list(fmap) == [2, 0]
    assert not np.array_equal(plain[1], fmap)                                 # the key order differs from the value order
    assert list(keys) == [1.0 + 0.5 * 6.0, 3.0] and best_value[0] == 4.0 and best_action[0] == 2
    assert list(out["value"]) == [1.0, 3.0]                                   # the slots hold the un-bootstrapped returns
    assert list(out["flags"]) == [planning.BEAM_VALID | planning.BEAM_LIVE, planning.BEAM_VALID]
    # the next level continues the true return: the leaf term is not carried along
    r2 = np.array([10.0, 20.0, 30.0, 7.0, 7.0, 7.0])
    cand = planning.beam_candidates(r2, np.zeros(6, np.uint8), 1, 2, 1, 0.5, out)
    assert list(cand["value"][:4]) == [1.0 + 0.5 * 10.0, 1.0 + 0.5 * 20.0, 1.0 + 0.5 * 30.0, 3.0]
    # an invalid candidate's key is NaN, whatever its leaf
    cand0 = planning.beam_candidates(r, q, 1, 2, 0, 1.0)
    assert np.isnan(planning.beam_keys(cand0, leaf, 0.5)[3:]).all()


def test_beam_boot_orders_every_root_by_beats_rule():
    """random levels with NaN leaves, ties and finished parents: within a root the kept keys never increase, NaN keys come last
    among the valid, and the kept set is what a per-root Python sort by (valid, key, index) keeps"""
    rng = np.random.default_rng(11)
    n_roots, width, level = 9, 4, 3
    r, q, slots = _level(rng, n_roots, width)
    leaf = np.round(rng.normal(size=3 * width * n_roots), 1).astype(np.float32)
    leaf[::7] = np.nan
    out, fmap, keys, best_value, _ = planning.beam_select_boot_ref(r, q, leaf, n_roots, width, level, 0.9, 0.81, slots)
    cand = planning.beam_candidates(r, q, n_roots, width, level, 0.9, slots)
    allkeys = planning.beam_keys(cand, leaf, 0.81)
    nc = 3 * width
    for root in range(n_roots):
        idx = list(range(root * nc, (root + 1) * nc))
        valid = [c for c in idx if cand["flags"][c] & planning.BEAM_VALID]
        numbers = sorted([c for c in valid if not np.isnan(allkeys[c])], key=lambda c: (-allkeys[c], c))
        order = numbers + [c for c in valid if np.isnan(allkeys[c])]
        want = (order + [-1] * width)[:width]
        assert list(fmap[root * width:(root + 1) * width]) == want
        kept = keys[root * width:(root + 1) * width]
        assert np.array_equal(kept[:len(order)][:width], allkeys[order[:width]], equal_nan=True)
        assert np.array_equal(best_value[root], kept[0], equal_nan=True)
        got_values = out["value"][root * width:(root + 1) * width]
        assert np.array_equal(got_values[:min(len(order), width)], cand["value"][order[:width]], equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------- C entry points
PTR, PTR2 = 1 << 20, 2 << 20                                # (never dereferenced: every call below is refused before any launch)


def test_select_branches_boot_refuses_bad_arguments():
    lib = _lib.load()
    names = ("reward_hist", "reason_hist", "first_action", "n_steps", "n_branch", "group", "gamma", "leaf", "values", "best_value",
             "best_action", "stream")
    ok = (PTR, PTR, PTR, 2, 18, 9, 0.99, PTR, PTR, PTR, PTR, None)

    def call(**kw):
        args = dict(zip(names, ok))
        args.update(kw)
        return lib.bsk_select_branches_boot(*[args[n] for n in names])

    for name in ("reward_hist", "reason_hist", "first_action", "best_action"):
        assert call(**{name: None}) == -1, name
    assert call(leaf=None) == -1
    assert b"leaf" in lib.bsk_last_error()
    assert call(n_steps=0) == -1 and call(n_branch=0) == -1 and call(group=0) == -1
    assert call(group=5) == -1
    assert b"multiple" in lib.bsk_last_error()


def test_beam_select_boot_refuses_bad_arguments():
    lib = _lib.load()
    names = ("reward", "reason", "n_roots", "width", "level", "weight", "boot_weight", "leaf", "d_in", "d_out", "map", "key", "best_value",
             "best_action", "stream")
    ok = (PTR, PTR, 4, 9, 1, 1.0, 0.99, PTR, PTR2, PTR, PTR, None, PTR, PTR, None)

    def call(**kw):
        args = dict(zip(names, ok))
        args.update(kw)
        return lib.bsk_beam_select_boot(*[args[n] for n in names])

    for name in ("reward", "reason", "d_out", "map", "best_value", "best_action"):
        assert call(**{name: None}) == -1, name
    assert call(d_in=None) == -1
    for width in (0, 82):
        assert call(width=width) == -1
    assert call(n_roots=0) == -1 and call(level=-1) == -1
    assert call(n_roots=2 ** 31 // 27 + 1) == -1
    for w in (float("nan"), float("inf")):
        assert call(weight=w) == -1
    assert call(d_in=PTR) == -1
    assert b"distinct" in lib.bsk_last_error()
    assert call(leaf=None) == -1
    assert b"leaf" in lib.bsk_last_error()
    for w in (float("nan"), float("inf"), float("-inf")):
        assert call(boot_weight=w) == -1
        assert b"boot_weight" in lib.bsk_last_error()


def test_policy_value_refuses_a_null_policy():
    """(a policy cannot exist without a device: the refusals that need one are in tests/test_gpu_planner_boot.py)"""
    lib = _lib.load()
    assert lib.bsk_policy_value(None, PTR, 64, 64, PTR, None) == -1
    assert b"NULL" in lib.bsk_last_error()
    assert lib.bsk_policy_value(None, None, 64, 64, None, None) == -1
    assert lib.bsk_policy_value(None, PTR, 8, 64, PTR, None) == -1 and lib.bsk_policy_value(None, PTR, 64, 0, PTR, None) == -1


# ------------------------------------------------------------------------------------------------------------- planner arguments
def _stand_in(value_hidden, device=0):
    """what the argument rules read of a DevicePolicy (one cannot be created without a device)"""
    return types.SimpleNamespace(spec=check_spec([16], "relu", value_hidden), device=device, value_enqueue=lambda *a: None)


def test_planners_refuse_a_bad_bootstrap_word():
    for word in ("sometimes", "", None, "EVERY", 1):
        with pytest.raises(ValueError):
            planning.BeamPlanner(None, width=3, horizon=2, substeps=10, bootstrap=word)
        with pytest.raises(ValueError):
            planning.check_bootstrap(word)
    assert planning.check_bootstrap("every") == "every" and planning.check_bootstrap("last") == "last"


def test_planners_refuse_a_policy_without_a_value_network():
    for make in (lambda p: planning.LookaheadPlanner(None, depth=2, substeps=10, value_policy=p),
                 lambda p: planning.BeamPlanner(None, width=3, horizon=2, substeps=10, value_policy=p)):
        with pytest.raises(ValueError, match="no value network"):
            make(_stand_in(None))
        with pytest.raises(TypeError):                  # (with a value network the rules pass: the root is refused next)
            make(_stand_in([16]))
    with pytest.raises(TypeError):
        planning.check_value_policy(object())


def test_planners_refuse_a_policy_on_another_device():
    with pytest.raises(ValueError, match="device 1"):
        planning.check_value_policy(_stand_in([16], device=1), 0)
    pol = _stand_in([16], device=2)
    assert planning.check_value_policy(pol, 2) is pol and planning.check_value_policy(None, 0) is None
