"""CPU: what the training log of the policy-gradient loop states without a device - ``pg_episodes_ref`` / ``pg_log_update_ref``
(include/bskgpu.h, bsk_pg_episodes; csrc/bsk_pglog.hip), the argument rules ``check_pg_episodes`` / ``check_pg_log``, and the
per-column walk of csrc/bsk_pglog.hpp itself, compiled for the HOST (tools/pg_episodes_host.cpp) under the address and
undefined-behaviour sanitizers and held to the restatement bit for bit, before a GPU runs it.

The restatement is held to a plain per-env Python loop with numpy.sum / min / max / var: counts and extremes EQUAL - the returns of
the ended episodes are the same f64 numbers on both sides -, the f64 sums and the explained variance within the bounds derived in
tests/_pg_log_bounds.py.  No case is skipped."""
import os
import subprocess

import numpy as np
import pytest

from _device_bits import same as _same
from _pg_log_bounds import explained_variance_bound, sum_bound
from _pg_log_cases import HOST_SHAPES, diag_case, episode_case
from basilisk_env_amd import _lib
from basilisk_env_amd import policy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COL = {name: c for c, name in enumerate(P.PG_LOG_COLUMNS)}
INTEGER_COLUMNS = (0, 5, 6, 7, 8, 9, 10, 11, 12)


def _plain(case):
    """one env after the other, one row after the other -> (returns, lengths, reasons of the ended episodes, new state)"""
    T, n = case["reward"].shape
    returns, lengths, reasons = [], [], []
    R_out, L_out = np.empty(n, np.float64), np.empty(n, np.int32)
    for j in range(n):
        R, L = float(case["state"][0][j]), int(case["state"][1][j])
        for t in range(T):
            R = R + float(case["reward"][t, j])
            L += 1
            if case["reason"][t, j]:
                returns.append(R)
                lengths.append(L)
                reasons.append(int(case["reason"][t, j]))
                R, L = 0.0, 0
        R_out[j], L_out[j] = R, L
    return np.array(returns, np.float64), np.array(lengths, np.int64), np.array(reasons, np.int64), (R_out, L_out)


def test_the_columns_are_named_once():
    assert P.PG_LOG_COLS == 26 == len(P.PG_LOG_COLUMNS) == len(set(P.PG_LOG_COLUMNS))
    assert P.PG_LOG_COLUMNS[16:20] == P.PG_STATS_COLUMNS and P.PG_LOG_COLUMNS[20:24] == P.FIT_STATS_COLUMNS
    assert COL["explained_variance"] == 14 and COL["grad_clipped"] == 25


@pytest.mark.parametrize("n,T", HOST_SHAPES)
def test_the_restatement_against_a_plain_loop(n, T):
    case = episode_case(T, n, 10 * n + T)
    row, (R, L) = P.pg_episodes_ref(**case)
    assert row.shape == (16,) and row.dtype == np.float64 and R.dtype == np.float64 and L.dtype == np.int32
    returns, lengths, reasons, (want_R, want_L) = _plain(case)
    assert _same(R, want_R) and np.array_equal(L, want_L)
    # counts and extremes: exact
    assert row[0] == returns.size and row[5] == lengths.sum()
    for b in range(4):
        assert row[6 + b] == ((reasons & (1 << b)) != 0).sum()
    for a in range(3):
        assert row[10 + a] == (case["action"] == a).sum()
    if returns.size:
        assert _same(row[3], returns.min()) and _same(row[4], returns.max())
    else:
        assert np.isnan(row[3]) and np.isnan(row[4])
    # the sums: within the bound of a reordered sum of the same terms
    e = case["ret"] - case["value"].astype(np.float64)
    for c, terms in ((1, returns), (2, returns * returns), (13, case["reward"]), (15, e * e)):
        bound = sum_bound(terms)
        print("column %d: |difference| %.3e, bound %.3e" % (c, abs(row[c] - terms.sum()), bound))
        assert abs(row[c] - terms.sum()) <= bound, c
    # the explained variance
    if T * n > 1:
        want = 1.0 - np.var(e) / np.var(case["ret"])
        bound = explained_variance_bound(case["ret"], e)
        print("explained variance %.6f: |difference| %.3e, bound %.3e" % (want, abs(row[14] - want), bound))
        assert bound < 1e-9 and abs(row[14] - want) <= bound
    else:
        assert np.isnan(row[14])                                # one sample: var_y == 0, PPO2's NaN


def test_two_rollouts_with_carried_state_are_the_one_they_make():
    n = 70
    whole = episode_case(6, n, 3)
    keys = ("reward", "reason", "action", "value", "ret")
    first, state = P.pg_episodes_ref(*[whole[k][:3] for k in keys], state=whole["state"])
    second, state = P.pg_episodes_ref(*[whole[k][3:] for k in keys], state=state)
    row, want = P.pg_episodes_ref(**whole)
    assert _same(state[0], want[0]) and np.array_equal(state[1], want[1])
    assert row[0] > 0
    for c in INTEGER_COLUMNS:
        assert first[c] + second[c] == row[c], c
    # ... and an episode that spans the cut is reported whole: the extremes of the two halves are those of the one
    assert min(first[3], second[3]) == row[3] and max(first[4], second[4]) == row[4]


def test_the_branches_of_the_restatement():
    case = episode_case(5, 65, 4)
    quiet = dict(case, reason=np.zeros_like(case["reason"]))
    row, (R, L) = P.pg_episodes_ref(**quiet)
    assert row[0] == 0 and np.isnan(row[3]) and np.isnan(row[4]) and row[1] == 0 and (row[6:10] == 0).all()
    assert np.array_equal(L, case["state"][1] + 5)             # the state grows
    every = dict(case, reason=np.full_like(case["reason"], 1))
    row, (R, L) = P.pg_episodes_ref(**every)
    assert row[0] == 5 * 65 and row[6] == 5 * 65 and (R == 0).all() and not np.signbit(R).any() and (L == 0).all()
    assert row[5] == (case["state"][1] + 1).sum() + 4 * 65
    two = dict(case, reason=np.where(case["reason"] != 0, 0x5, 0).astype(np.uint8))
    row, _ = P.pg_episodes_ref(**two)
    assert row[0] > 0 and row[6] == row[0] == row[8] and row[7] == 0 and row[9] == 0
    bare = {k: v for k, v in case.items() if k not in ("action", "value", "ret")}
    row, _ = P.pg_episodes_ref(**bare)
    assert (row[10:13] == 0).all() and np.isnan(row[14]) and _same(row[15], np.float64(0.0))
    odd = dict(case, action=np.where(case["action"] == 2, 7, case["action"]).astype(np.int32))
    row, _ = P.pg_episodes_ref(**odd)
    assert row[12] == 0 and row[10] + row[11] == (case["action"] != 2).sum()
    flat = dict(case, ret=np.full_like(case["ret"], 1.5))
    row, _ = P.pg_episodes_ref(**flat)
    assert np.isnan(row[14]) and row[15] > 0
    fresh, _ = P.pg_episodes_ref(**dict(case, state=None))
    zeros, _ = P.pg_episodes_ref(**dict(case, state=(np.zeros(65), np.zeros(65, np.int32))))
    assert _same(fresh, zeros)


def test_log_update_ref_sums_the_rows_from_the_first():
    diag, norms = diag_case(9, 4, 1)
    out = P.pg_log_update_ref(diag, norms)
    assert out.shape == (10,) and out.dtype == np.float64
    s = diag[0].copy()
    for r in range(1, 9):
        s = s + diag[r]
    assert _same(out[:8], s) and abs(out[8] - norms[:, 0].sum()) <= sum_bound(norms[:, 0])
    assert norms[0, 1] == 1.0 and out[9] == (norms[:, 1] < 1.0).sum() and 0 < out[9] < 4
    bare = P.pg_log_update_ref(diag[:1])
    assert _same(bare[:8], diag[0]) and _same(bare[8:], np.zeros(2))
    minus = P.pg_log_update_ref(np.full((1, 8), -0.0))
    assert np.signbit(minus[:8]).all()                          # from the first row, not from +0.0
    for bad in (np.zeros((0, 8)), np.zeros((2, 7)), np.zeros(8)):
        with pytest.raises(ValueError):
            P.pg_log_update_ref(bad)
    with pytest.raises(ValueError):
        P.pg_log_update_ref(diag, np.zeros((0, 2)))


def test_the_ring_table_is_the_written_slots_oldest_first():
    gen = np.array([3, 4, 2], np.uint64)
    rows = np.arange(3 * 26, dtype=np.float64).reshape(3, 26)
    it, out = P.pg_log_table_ref(gen, rows)
    assert list(it) == [2, 3, 4] and _same(out, rows[[2, 0, 1]])
    gen[1] = P.ES_LOG_EMPTY
    it, out = P.pg_log_table_ref(gen, rows)
    assert list(it) == [2, 3] and _same(out, rows[[2, 0]])
    it, out = P.pg_log_table_ref(np.full(2, P.ES_LOG_EMPTY, np.uint64), rows[:2])
    assert it.shape == (0,) and out.shape == (0, 26)


def test_the_argument_rules():
    assert P.check_pg_episodes(8, 65, 70, 3) == (8, 65, 70, 3)
    assert P.check_pg_episodes(2 ** 15, 2 ** 16, 2 ** 16, 1, True, True) == (2 ** 15, 2 ** 16, 2 ** 16, 1)
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 2, 1, 1), (1, 1, 1, 0), (2 ** 15, 2 ** 16, 2 ** 16 + 1, 1), (1.0, 1, 1, 1), (True, 1, 1, 1),
                (1, 1, 1, 1, True, False), (1, 1, 1, 1, False, True)):
        with pytest.raises(ValueError):
            P.check_pg_episodes(*bad)
    assert P.check_pg_log(9, 3) == (9, 3, None) and P.check_pg_log(1, 1, 4) == (1, 1, 4)
    for bad in ((0, 1), (1, 0), (1, 1, 0), (1.0, 1), (1, True)):
        with pytest.raises(ValueError):
            P.check_pg_log(*bad)
    for n in (1, 63, 64, 65, 4097, 65536):
        assert P.pg_episodes_work_bytes(n) == 8 * 19 * ((n + 63) // 64)
    with pytest.raises(ValueError):
        P.pg_episodes_work_bytes(0)


def test_the_symbols_are_declared_and_exported():
    lib = _lib.load()
    for name in ("bsk_pg_episodes_work_bytes", "bsk_pg_episodes", "bsk_pg_log_update", "bsk_pg_log_advance"):
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(lib, name), name
    for n in (1, 64, 65, 65536):
        assert lib.bsk_pg_episodes_work_bytes(n) == P.pg_episodes_work_bytes(n)
    assert lib.bsk_pg_episodes_work_bytes(0) == 0
    # refused before anything is launched: no device is needed to be told so
    assert lib.bsk_pg_episodes(None, None, None, None, None, 1, 1, 1, None, None, None, None, 1, None, None) == -1
    assert lib.bsk_pg_log_update(None, 1, None, 0, None, 1, None, None) == -1
    assert lib.bsk_pg_log_advance(None, 1, None, None) == -1


def _hex64(a):
    return ["%016x" % int(b) for b in np.ascontiguousarray(a, np.float64).view(np.uint64).reshape(-1)]


def test_the_device_walk_compiled_for_the_host_is_the_restatement(tmp_path):
    """csrc/bsk_pglog.hpp's pg_episode_walk as the GPU will run it - batches of eight rows, the tail, strided columns - under the
    address and undefined-behaviour sanitizers of the host compiler: its 19 accumulators and the new state of every column equal
    what the restatement holds in front of the trees, in every bit."""
    exe = tmp_path / "pg_episodes_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DBSK_PGLOG_HOST", "-I", os.path.join(ROOT, "basilisk_env_amd", "csrc"),
                           os.path.join(ROOT, "tools", "pg_episodes_host.cpp"), "-o", str(exe)])
    for n, T in HOST_SHAPES:
        case = episode_case(T, n, 10 * n + T)
        for with_action, with_value in ((True, True), (False, False)):
            lines = ["%s %d" % (r, l) for r, l in zip(_hex64(case["state"][0]), case["state"][1])]
            cells = zip(_hex64(case["reward"]), case["reason"].reshape(-1), case["action"].reshape(-1),
                        ["%08x" % int(b) for b in case["value"].view(np.uint32).reshape(-1)], _hex64(case["ret"]))
            lines += ["%s %d %d %s %s" % c for c in cells]
            out = subprocess.run([str(exe), str(T), str(n), str(n + 5), str(int(with_action)), str(int(with_value))],
                                 input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stderr
            got = [line.split() for line in out.stdout.splitlines()]
            assert len(got) == n and all(len(g) == 21 for g in got)
            s, mn, mx, k, (R, L) = P.pg_episodes_walk_ref(case["reward"], case["reason"], case["action"] if with_action else None,
                                                          case["value"] if with_value else None, case["ret"] if with_value else None,
                                                          case["state"])
            f = np.array([[int(w, 16) for w in g[:9] + g[19:20]] for g in got], np.uint64)
            i = np.array([[int(w) for w in g[9:19] + g[20:21]] for g in got], np.int64)
            want_f = np.concatenate([s, mn[None], mx[None], R[None]]).T
            assert np.array_equal(f, np.ascontiguousarray(want_f).view(np.uint64)), (n, T, with_action, with_value)
            assert np.array_equal(i, np.concatenate([k, L[None].astype(np.int64)]).T), (n, T, with_action, with_value)
