"""CPU: the restatements tests/test_gpu_pg_walks.py holds the column walks of the policy-gradient loop to - ``gae_ref``,
``reward_norm_ref``, ``pg_episodes_ref``, ``pg_log_update_ref``, ``adv_normalize_ref`` (basilisk_env_amd/policy_ref.py) - at the
shapes of tests/_pg_walk_cases.py, before a kernel is compared with them.

Each is held to a plain loop over Python floats - one column after the other, one row after the other, then the 64-lane tree and
the join of the partial rows written out lane by lane - that shares no code with the restatement and repeats the definition of
include/bskgpu.h in its own order of operations.  A Python float is an IEEE double and every operation on it is rounded on its own,
so the comparison is an equality of bits: there is no tolerance in this file.  At 513 envs the GAE loop runs on every fourth
column and those around the workgroup edges; everything else runs on every column.  The file also asserts what the constructions of
the cases promise - an end on the last row, on row 0, a wave whose one env alone ends an episode, and so on."""
import math

import numpy as np
import pytest

from _device_bits import same as _same
from _pg_cond_bounds import adv_case
from _pg_log_cases import diag_case
from _pg_walk_cases import (GAE_COEFS, GAE_KINDS, GAE_N, GAE_T, GRID_SHAPES, LAP_SHAPES, LOG_UPDATE_NORMS, LOG_UPDATE_ROWS, LOOP, ROW_SHAPES,
                            SEQUENCE_N, SEQUENCE_T, STALE_N, WHAT, episode_work_ref, gae_kind, gae_placement, gae_poisoned, gae_reach,
                            last_wave_case, sequence_cases, tag, walk_episode_case, walk_reward_case, waves)
from _reward_norm_cases import CLIP, EPS, GAMMA
from basilisk_env_amd import policy as P

NAN = float("nan")


# ------------------------------------------------------------------------------------------------------------------ the plain order
def _tree(v):
    """64 lanes -> lane 0: lane l takes lane l + stride, stride 32 .. 1"""
    v = list(v)
    assert len(v) == 64
    for stride in (32, 16, 8, 4, 2, 1):
        for l in range(stride):
            v[l] = v[l] + v[l + stride]
    return v[0]


def _pick(m, x, greatest):
    return x if ((x > m) if greatest else (x < m)) or m != m else m


def _pick_tree(v, greatest):
    v = list(v)
    for stride in (32, 16, 8, 4, 2, 1):
        for l in range(stride):
            v[l] = _pick(v[l], v[l + stride], greatest)
    return v[0]


def _join(parts):
    """lane l the entries l, l + 64, ... ascending FROM the first (+0.0 with none), then the tree"""
    lanes = [0.0] * 64
    for w, v in enumerate(parts):
        lanes[w % 64] = v if w < 64 else lanes[w % 64] + v
    return _tree(lanes)


def _join_pick(parts, greatest):
    lanes = [NAN] * 64
    for w, v in enumerate(parts):
        lanes[w % 64] = _pick(lanes[w % 64], v, greatest)
    return _pick_tree(lanes, greatest)


def _per_wave(lane_values, n, fill, join):
    """per-lane values of n columns -> one value per wave; the lanes at and above n bring ``fill``"""
    W = waves(n)
    full = list(lane_values) + [fill] * (W * 64 - n)
    return [join(full[64 * w:64 * w + 64]) for w in range(W)]


def _moments(s, s2, count):
    N = float(count)
    mean = s / N
    v = s2 / N - mean * mean
    return mean, (v if v > 0.0 else 0.0)


def _f64_bits(x):
    return np.array(x, np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------------ bsk_reward_norm
def _plain_reward_norm(case, update, gamma=GAMMA, eps=EPS, clip=CLIP):
    """-> (out f64 (T, n), words u64 (8,), ret_run f64 (n,), work u64 (W, 3) or None)"""
    reward, reason = case["reward"], case["reason"]
    T, n = reward.shape
    f = [float(x) for x in case["state"].view(np.float64)]
    count, calls = int(case["state"][2]), int(case["state"][6])
    R_out, work = [float(x) for x in case["ret_run"]], None
    words = case["state"].copy()
    if update:
        a1, a2, k = [], [], []
        for j in range(n):
            R, s1, s2 = R_out[j], 0.0, 0.0
            rew, why = reward[:, j].tolist(), reason[:, j].tolist()
            for t in range(T):
                R = gamma * R
                R = R + rew[t]
                s1 = s1 + R
                s2 = s2 + R * R
                if why[t] != 0:
                    R = 0.0
            R_out[j] = R
            a1.append(s1)
            a2.append(s2)
            k.append(T)
        p1, p2 = _per_wave(a1, n, 0.0, _tree), _per_wave(a2, n, 0.0, _tree)
        pk = _per_wave(k, n, 0, sum)
        work = np.empty((waves(n), 3), np.uint64)
        work[:, 0], work[:, 1], work[:, 2] = _f64_bits(p1), _f64_bits(p2), np.array(pk, np.uint64)
        s, s2, count = f[0] + _join(p1), f[1] + _join(p2), count + sum(pk)
        mean, var = _moments(s, s2, count)
        words = np.r_[_f64_bits([s, s2]), np.array([count], np.uint64), _f64_bits([mean, var, math.sqrt(var + eps)]),
                      np.array([calls + 1, 0], np.uint64)]
        f[5] = math.sqrt(var + eps)
    d = f[5] if count != 0 else 1.0
    out = np.empty((T, n), np.float64)
    for t in range(T):
        row = reward[t].tolist()
        for j in range(n):
            y = row[j] / d
            out[t, j] = clip if y > clip else (-clip if y < -clip else y)
    return out, words, np.array(R_out, np.float64), work


def _check_reward(case, update, where):
    got = P.reward_norm_ref(case["reward"], case["reason"], GAMMA, EPS, CLIP, update, case["state"], case["ret_run"], with_work=True)
    want = _plain_reward_norm(case, update)
    for name, a, b in zip(("out", "state", "ret_run"), got, want):
        assert _same(a, b), (where, name)
    assert (got[3] is None and want[3] is None) if not update else _same(got[3], want[3]), (where, "work")
    return got


@pytest.mark.parametrize("n,T", ROW_SHAPES + GRID_SHAPES + LAP_SHAPES)
def test_reward_norm_ref_equals_a_plain_loop(n, T):
    case = walk_reward_case(n, T)
    out, words, R, work = _check_reward(case, 1, tag(n, T))
    assert int(words[2]) == int(case["state"][2]) + T * n and int(words[6]) == 4 and work.shape == (waves(n), 3)
    assert (out == CLIP).any() and (out == -CLIP).any() and (np.abs(out) < CLIP).any(), tag(n, T)
    if (n, T) in GRID_SHAPES:
        frozen = _check_reward(case, 0, tag(n, T))
        assert _same(frozen[1], case["state"]) and _same(frozen[2], case["ret_run"]) and not _same(frozen[0], out)
        # the rows only a second or third trip of the apply's row stride reaches hold something a stale output would not
        assert T == 1024 or not _same(out[1024:], case["reward"][1024:]), tag(n, T)
    if T > 8:
        assert (case["reason"][8:] != 0).any() and (case["reason"][:8] != 0).any(), tag(n, T)      # ends in the first batch and behind it


def test_reward_norm_ref_chains_three_calls_and_ignores_stale_work_rows():
    cases = sequence_cases("reward")
    assert [c["reward"].shape for c in cases] == [(T, SEQUENCE_N) for T in SEQUENCE_T] and SEQUENCE_T == (9, 16, 1)
    state, R = cases[0]["state"], cases[0]["ret_run"]
    for i, c in enumerate(cases):
        c = dict(c, state=state, ret_run=R)
        _, state, R, _ = _check_reward(c, 1, ("call", i))
    assert int(state[6]) == 3 + 3 and int(state[2]) == int(cases[0]["state"][2]) + sum(SEQUENCE_T) * SEQUENCE_N
    assert waves(STALE_N[0]) == 5 and waves(STALE_N[1]) == 2          # three rows of the larger call lie behind the smaller one's


# ------------------------------------------------------------------------------------------------------------------ bsk_pg_episodes
def _plain_episodes(case, with_action=True, with_value=True):
    """-> (row f64 (16,), ep_return f64 (n,), ep_len i32 (n,), work u64 (W, 19))"""
    T, n = case["reward"].shape
    lanes_s, lanes_mn, lanes_mx, lanes_k = [[] for _ in range(7)], [], [], [[] for _ in range(10)]
    R_out, L_out = [], []
    for j in range(n):
        R, L = float(case["state"][0][j]), int(case["state"][1][j])
        s, mn, mx, k = [0.0] * 7, NAN, NAN, [0] * 10
        rew, why = case["reward"][:, j].tolist(), case["reason"][:, j].tolist()
        act = case["action"][:, j].tolist()
        val, ret = case["value"][:, j].astype(np.float64).tolist(), case["ret"][:, j].tolist()
        for t in range(T):
            R = R + rew[t]
            L = L + 1
            s[2] = s[2] + rew[t]
            k[9] += 1
            if with_action and 0 <= act[t] <= 2:
                k[6 + act[t]] += 1
            if with_value:
                y = ret[t]
                e = y - val[t]
                s[3] = s[3] + y
                s[4] = s[4] + y * y
                s[5] = s[5] + e
                s[6] = s[6] + e * e
            if why[t] != 0:
                s[0] = s[0] + R
                s[1] = s[1] + R * R
                mn, mx = _pick(mn, R, False), _pick(mx, R, True)
                k[0] += 1
                k[1] += L
                for b in range(4):
                    k[2 + b] += 1 if why[t] & (1 << b) else 0
                R, L = 0.0, 0
        R_out.append(R)
        L_out.append(L)
        for c in range(7):
            lanes_s[c].append(s[c])
        lanes_mn.append(mn)
        lanes_mx.append(mx)
        for c in range(10):
            lanes_k[c].append(k[c])
    W = waves(n)
    part_s = [_per_wave(lanes_s[c], n, 0.0, _tree) for c in range(7)]
    part_mn = _per_wave(lanes_mn, n, NAN, lambda v: _pick_tree(v, False))
    part_mx = _per_wave(lanes_mx, n, NAN, lambda v: _pick_tree(v, True))
    part_k = [_per_wave(lanes_k[c], n, 0, sum) for c in range(10)]
    work = np.empty((W, 19), np.uint64)
    for c in range(7):
        work[:, c] = _f64_bits(part_s[c])
    work[:, 7], work[:, 8] = _f64_bits(part_mn), _f64_bits(part_mx)
    for c in range(10):
        work[:, 9 + c] = np.array(part_k[c], np.uint64)
    tot = [_join(part_s[c]) for c in range(7)]
    cnt = [sum(part_k[c]) for c in range(10)]
    row = [float(cnt[0]), tot[0], tot[1], _join_pick(part_mn, False), _join_pick(part_mx, True), float(cnt[1])]
    row += [float(x) for x in cnt[2:9]] + [tot[2]]
    ev = NAN
    if with_value:
        _, var_y = _moments(tot[3], tot[4], cnt[9])
        _, var_e = _moments(tot[5], tot[6], cnt[9])
        if var_y != 0.0:
            ev = 1.0 - var_e / var_y
    row += [ev, tot[6]]
    return np.array(row, np.float64), np.array(R_out, np.float64), np.array(L_out, np.int32), work


KEYS = ("reward", "reason", "action", "value", "ret")


def _check_episodes(case, where, with_action=True, with_value=True):
    keys = tuple(k for k in KEYS if (with_action or k != "action") and (with_value or k not in ("value", "ret")))
    row, (R, L) = P.pg_episodes_ref(**{k: case[k] for k in keys + ("state",)})
    want_row, want_R, want_L, want_work = _plain_episodes(case, with_action, with_value)
    assert _same(row, want_row), (where, row, want_row)
    assert _same(R, want_R) and _same(L, want_L), where
    work = episode_work_ref(case, keys)
    assert _same(work, want_work), (where, np.argwhere(work != want_work)[:4])
    return row, work


@pytest.mark.parametrize("n,T", ROW_SHAPES + LAP_SHAPES)
def test_pg_episodes_ref_equals_a_plain_loop(n, T):
    case = walk_episode_case(n, T)
    row, work = _check_episodes(case, tag(n, T))
    assert row[0] == (case["reason"] != 0).sum() > 0 and row[10:13].sum() == T * n and np.isfinite(row[14]) and work.shape == (waves(n), 19)
    if (n, T) in ((65, 17), (8321, 9)):
        for with_action, with_value in ((False, True), (True, False), (False, False)):
            r, _ = _check_episodes(case, (tag(n, T), with_action, with_value), with_action, with_value)
            assert np.isnan(r[14]) == (not with_value) and (r[10:13].sum() == 0) == (not with_action)
    if T > 8:
        assert (case["reason"][8:] != 0).any() and (case["reason"][:8] != 0).any(), tag(n, T)


def test_the_last_waves_one_env_alone_ends_episodes():
    case = last_wave_case()
    n, T = LAP_SHAPES[-1]
    assert n % 64 == 1 and waves(n) == 131
    ends = np.argwhere(case["reason"] != 0)
    assert len(ends) == 3 and (ends[:, 1] == n - 1).all() and sorted(ends[:, 0]) == [2, 5, 8]
    row, work = _check_episodes(case, "only the last wave ends an episode")
    f = work.view(np.float64)
    assert np.isnan(f[:130, 7:9]).all() and np.isfinite(f[130, 7:9]).all() and not work[:130, 9].any() and work[130, 9] == 3
    assert row[0] == 3 and row[3] <= row[4] and _same(row[3:5], f[130, 7:9]) and row[5] == work[130, 10] > 0
    assert row[6] == 1 and row[7] == 0 and row[8] == 1 and row[9] == 1


def test_pg_episodes_ref_chains_three_calls():
    cases = sequence_cases("episode")
    state = cases[0]["state"]
    for i, c in enumerate(cases):
        c = dict(c, state=state)
        _check_episodes(c, ("call", i))
        _, state = P.pg_episodes_ref(**{k: c[k] for k in KEYS + ("state",)})
    assert (state[1] >= 0).all() and (state[1] > 0).any() and (state[1] == 0).any()      # the one row of the last call ended some


@pytest.mark.parametrize("n_norms", LOG_UPDATE_NORMS)
@pytest.mark.parametrize("n_rows", LOG_UPDATE_ROWS)
def test_pg_log_update_ref_equals_a_plain_loop(n_rows, n_norms):
    diag, norms = diag_case(n_rows, n_norms or 1, n_rows + (n_norms or 0))
    norms = norms if n_norms else None
    want = []
    for c in range(8):
        col = diag[:, c].tolist()
        s = col[0]
        for v in col[1:]:
            s = s + v
        want.append(s)
    total, clipped = 0.0, 0
    if norms is not None:
        col = norms[:, 0].tolist()
        total = col[0]
        for v in col[1:]:
            total = total + v
        clipped = sum(1 for x in norms[:, 1].tolist() if x < 1.0)
        assert norms.shape == (n_norms, 2) and norms[0, 1] == 1.0 and (n_norms == 1 or 0 < clipped < n_norms)
    assert _same(P.pg_log_update_ref(diag, norms), np.array(want + [total, float(clipped)], np.float64)), (n_rows, n_norms)


# ------------------------------------------------------------------------------------------------------------------ bsk_adv_normalize
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n,rows", LAP_SHAPES)
def test_adv_normalize_ref_equals_a_plain_loop_at_the_lap_shapes(n, rows, masked):
    eps = 1e-8
    adv, alive = adv_case(rows, n, 10 * n + rows, masked=masked)
    a1, a2, k = [], [], []
    for j in range(n):
        x = adv[:, j].astype(np.float64).tolist()
        on = [True] * rows if alive is None else (alive[:, j] != 0).tolist()
        s1, s2 = 0.0, 0.0
        for t in range(rows):
            xd = x[t] if on[t] else 0.0
            s1 = s1 + xd
            s2 = s2 + xd * xd
        a1.append(s1)
        a2.append(s2)
        k.append(sum(on))
    N = sum(k)
    mean, var = _moments(_join(_per_wave(a1, n, 0.0, _tree)), _join(_per_wave(a2, n, 0.0, _tree)), N)
    sd = math.sqrt(var)
    inv = 1.0 / (sd + eps)
    want = np.zeros((rows, n), np.float32)
    for t in range(rows):
        for j in range(n):
            if alive is None or alive[t, j]:
                want[t, j] = np.float32((float(adv[t, j]) - mean) * inv)
    out, mom = P.adv_normalize_ref(adv, alive, eps)
    assert _same(mom, np.array([mean, sd, inv, float(N)], np.float64)), (tag(n, rows), masked)
    assert _same(out, want) and (N == rows * n) == (not masked), (tag(n, rows), masked)


# ------------------------------------------------------------------------------------------------------------------ bsk_gae
def _plain_gae(reward, reason, value, last, gamma, lam, cols):
    T = reward.shape[0]
    adv, ret = np.empty((T, len(cols)), np.float32), np.empty((T, len(cols)), np.float64)
    gl = gamma * lam
    for i, j in enumerate(cols):
        rew, why, v = reward[:, j].tolist(), reason[:, j].tolist(), value[:, j].astype(np.float64).tolist()
        carry, next_v = 0.0, 0.0 if last is None else float(last[j])
        for t in range(T - 1, -1, -1):
            if why[t] == 0:
                delta = (rew[t] + gamma * next_v) - v[t]
                carry = delta + gl * carry
            else:
                carry = rew[t] - v[t]
            adv[t, i] = np.float32(carry)
            ret[t, i] = carry + v[t]
            next_v = v[t]
    return adv, ret


@pytest.mark.parametrize("n", GAE_N)
@pytest.mark.parametrize("T", GAE_T)
def test_gae_ref_equals_a_plain_loop_and_the_cut_shows(T, n):
    reward, reason, value, last = gae_placement(T, n)
    cols = list(range(n)) if n < 500 else sorted(set(range(0, n, 4)) | {254, 255, 256, 257, 510, 511, 512})
    # what the construction promises: every kind of column in every workgroup, an end on the last row and on row 0
    for lo in range(0, n - 6, 256):
        assert {gae_kind(c) for c in range(lo, min(lo + 256, n))} == set(GAE_KINDS)
    by = {kind: [c for c in range(n) if gae_kind(c) == kind] for kind in GAE_KINDS}
    assert (reason[T - 1, by["last"]] != 0).all() and not reason[:T - 1, by["last"]].any()
    assert (reason[0, by["first"]] != 0).all() and not reason[1:, by["first"]].any()
    assert (reason[:, by["every"]] != 0).all() and not reason[:, by["never"]].any()
    assert (reason[[0, T - 1]][:, by["first_and_last"]] != 0).all() and (reason[T // 2, by["middle"]] != 0).all()
    assert set(np.unique(reason)) == {0, 1, 2, 4, 8}
    reach = gae_reach(reason)
    assert not reach[:, by["last"] + by["every"] + by["first_and_last"]].any() and reach[:, by["never"]].all()
    assert reach[1:, by["first"]].all() and not reach[0, by["first"]].any()
    for gamma, lam in GAE_COEFS:
        both = []
        for x in (None, last):
            adv, ret = P.gae_ref(reward, reason, value, x, gamma, lam)
            want_adv, want_ret = _plain_gae(reward, reason, value, x, gamma, lam, cols)
            assert _same(adv[:, cols], want_adv) and _same(ret[:, cols], want_ret), (T, n, gamma, lam, x is not None)
            both.append((adv, ret))
        # the cut: the two estimates differ where last_value can reach and nowhere else
        d_adv, d_ret = both[0][0] != both[1][0], both[0][1] != both[1][1]
        if gamma == 0.0:
            assert not d_adv.any() and not d_ret.any()
        else:
            assert np.array_equal(d_ret, reach), (T, n, gamma, lam)
            assert not (d_adv & ~reach).any() and d_adv[T - 1][reach[T - 1]].all() and d_adv.sum() >= 0.99 * reach.sum()


def test_the_poisoned_columns_are_one_per_wave():
    for n in GAE_N:
        reward, reason, value, _ = gae_placement(9, n)
        r2, v2, cols = gae_poisoned(reward, value)
        assert len(cols) == waves(n) and np.array_equal(cols // 64, np.arange(waves(n))) and len(set(cols % 64)) == waves(n)
        bad = ~np.isfinite(r2) | ~np.isfinite(v2)
        assert bad.sum() == waves(n) and np.array_equal(np.flatnonzero(bad.any(axis=0)), cols)
        kinds = np.where(~np.isfinite(r2), r2, np.where(~np.isfinite(v2), v2.astype(np.float64), 0.0))[bad]
        assert np.isnan(kinds).any() and (kinds == np.inf).any() and (kinds == -np.inf).any()
        clean, dirty = P.gae_ref(reward, reason, value, None, 0.97, 0.9), P.gae_ref(r2, reason, v2, None, 0.97, 0.9)
        keep = np.setdiff1d(np.arange(n), cols)
        assert _same(clean[0][:, keep], dirty[0][:, keep]) and _same(clean[1][:, keep], dirty[1][:, keep])
        assert not np.isfinite(dirty[1][:, cols]).all()


# ------------------------------------------------------------------------------------------------------------------ the tables
def test_every_shape_is_named_and_is_what_it_says():
    assert set(WHAT) == set(ROW_SHAPES + GRID_SHAPES + LAP_SHAPES)
    assert [(T // 8, T % 8) for _, T in ROW_SHAPES] == [(1, 0), (2, 0), (2, 1), (3, 0)] and all(n == 65 for n, _ in ROW_SHAPES)
    assert [(T - 1) // 1024 + 1 for _, T in GRID_SHAPES] == [1, 2, 3]          # trips of row 0's threads over a grid of 1 024 rows
    assert [waves(n) for n, _ in LAP_SHAPES] == [64, 128, 131] and LAP_SHAPES[-1][0] % 64 == 1
    assert [(T // 4, T % 4) for T in GAE_T] == [(1, 0), (1, 1), (2, 0), (2, 1), (8, 1)]
    assert [(n - 1) // 256 + 1 for n in GAE_N] == [1, 1, 2, 3] and [n % 256 for n in GAE_N] == [255, 0, 1, 1]
    L = LOOP
    assert L["n_envs"] % 64 and L["n_steps"] // 8 == 2 and L["n_steps"] % 8 and L["n_steps"] % L["minibatches"] == 0
    assert L["iterations"] > L["log_capacity"]                                 # the ring wraps
    P.check_pg_loop(L["n_steps"], L["gamma"], L["lam"], 0.2, 0.01, L["epochs"], L["minibatches"], 1)
