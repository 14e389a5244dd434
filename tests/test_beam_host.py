"""CPU: the beam planner's host-side pieces (basilisk_env_amd/planning.py) - the numpy statement of bsk_beam_select's level rule
that the GPU tests hold the kernel to, held here to an exhaustive search and a greedy walk over synthetic trees of rewards - its
argument checks, bsk_beam_select's refusals, and that the planner fails loudly without a device."""
import functools
import os

import numpy as np
import pytest

from basilisk_env_amd import _lib, planning


def _tree(rng, n_roots, H):
    """Rewards and reasons on the nodes of one 3-ary tree per root: node (t, prefix) is step t of every sequence whose first t + 1
    actions are the base-3 digits of `prefix` (lowest digit first), the action_table order.  Quantised rewards (exact ties),
    NaNs, and endings at every depth."""
    r = [np.round(rng.normal(size=(n_roots, 3 ** (t + 1))), 1) for t in range(H)]
    q = [((rng.random((n_roots, 3 ** (t + 1))) < 0.15) * rng.integers(1, 16, (n_roots, 3 ** (t + 1)))).astype(np.uint8) for t in range(H)]
    for t in range(H):
        r[t][rng.random(r[t].shape) < 0.04] = np.nan
    return r, q


def _histories(r, q, n_roots, H):
    """the tree as LookaheadPlanner's histories: branch b = root * 3^H + k takes base-3 digit t of k at step t"""
    k = np.arange(3 ** H)
    rh = np.stack([r[t][:, k % 3 ** (t + 1)].ravel() for t in range(H)])
    qh = np.stack([q[t][:, k % 3 ** (t + 1)].ravel() for t in range(H)])
    return rh, qh


def _beam(r, q, n_roots, width, H, gamma):
    """beam_select_ref iterated over the tree: every slot remembers its prefix, forked back through the level's map"""
    w = planning.level_weights(gamma, H)
    ns = n_roots * width
    c = np.arange(3 * ns)
    root = c // (3 * width)
    prefix = np.zeros(ns, dtype=np.int64)
    slots = None
    for t in range(H):
        cp = prefix[c // 3] + (c % 3) * 3 ** t
        cp = np.where(cp < 3 ** (t + 1), cp, 0)          # (children of stale slots are invalid: any node will do)
        slots, fmap, bv, ba = planning.beam_select_ref(r[t][root, cp], q[t][root, cp], n_roots, width, t, w[t], slots)
        prefix = np.where(fmap >= 0, cp[np.maximum(fmap, 0)], prefix)
    return slots, fmap, bv, ba


@pytest.mark.parametrize("gamma", [1.0, 0.99])
@pytest.mark.parametrize("H", [1, 2, 3, 4])
def test_full_width_beam_equals_the_exhaustive_search(H, gamma):
    rng = np.random.default_rng(10 * H + int(gamma * 100))
    n_roots = 40
    r, q = _tree(rng, n_roots, H)
    slots, _, bv, ba = _beam(r, q, n_roots, 3 ** H, H, gamma)
    values = planning.branch_values(*_histories(r, q, n_roots, H), gamma).reshape(n_roots, 3 ** H)
    best, want = planning.select_best(values.ravel(), 3 ** H)
    assert np.array_equal(bv, want, equal_nan=True)
    for i in range(n_roots):                              # the first action lies in the exhaustive arg-max set
        v = values[i]
        arg = np.flatnonzero((v == want[i]) | (np.isnan(v) & np.isnan(want[i])))
        assert ba[i] in set(arg % 3)
    # every kept sequence has the value of one of the exhaustive branches
    for i in range(n_roots):
        kept = slots["value"].reshape(n_roots, -1)[i][(slots["flags"].reshape(n_roots, -1)[i] & planning.BEAM_VALID) != 0]
        assert np.isin(kept[~np.isnan(kept)], values[i]).all()


def _greedy(r, q, n_roots, H, gamma):
    w = planning.level_weights(gamma, H)
    out_v, out_a = [], []
    for i in range(n_roots):
        v, live, prefix, first = 0.0, True, 0, None
        for t in range(H):
            if not live:
                continue                                  # a finished sequence continues with action 0 and keeps its value
            best = None
            for a in range(3):
                node = prefix + a * 3 ** t
                val = v + w[t] * r[t][i, node] if t else 0.0 + w[t] * r[t][i, node]
                key = (np.isnan(val), -val if not np.isnan(val) else 0.0, a)
                if best is None or key < best[0]:
                    best = (key, val, a, node)
            _, v, a, prefix = best
            live = q[t][i, prefix] == 0
            first = a if first is None else first
        out_v.append(v)
        out_a.append(first)
    return np.array(out_v), np.array(out_a)


@pytest.mark.parametrize("gamma", [1.0, 0.9])
def test_width_one_is_a_greedy_walk(gamma):
    rng = np.random.default_rng(5)
    n_roots, H = 60, 4
    r, q = _tree(rng, n_roots, H)
    _, _, bv, ba = _beam(r, q, n_roots, 1, H, gamma)
    gv, ga = _greedy(r, q, n_roots, H, gamma)
    assert np.array_equal(bv, gv, equal_nan=True)
    assert np.array_equal(ba, ga)


def test_a_finished_parent_yields_one_child():
    width, n_roots = 3, 2
    slots = np.zeros(n_roots * width, dtype=planning.BEAM_SLOT)
    slots["value"] = [5.0, 4.0, 3.0, 2.0, 1.0, np.nan]
    slots["first"] = [2, 1, 0, 1, 2, -1]
    slots["flags"] = [planning.BEAM_VALID, planning.BEAM_VALID | planning.BEAM_LIVE, planning.BEAM_VALID,
                      planning.BEAM_LIVE, planning.BEAM_VALID | planning.BEAM_LIVE, 0]     # (live without valid: no sequence)
    reward = np.full(3 * width * n_roots, 10.0)
    reward[3], reward[5] = -20.0, 0.0
    reason = np.zeros(3 * width * n_roots, dtype=np.uint8)
    cand = planning.beam_candidates(reward, reason, n_roots, width, 1, 0.5, slots)
    valid = (cand["flags"] & planning.BEAM_VALID) != 0
    assert list(np.flatnonzero(valid)) == [0, 3, 4, 5, 6, 12, 13, 14]
    assert cand["value"][0] == 5.0 and cand["value"][6] == 3.0              # finished: the value stays, no reward added
    assert not (cand["flags"][[0, 6]] & planning.BEAM_LIVE).any() and (cand["flags"][[3, 4, 5]] & planning.BEAM_LIVE).all()
    assert list(cand["first"][[0, 3, 6, 12]]) == [2, 1, 0, 2] and (cand["first"][~valid] == -1).all()
    assert np.isnan(cand["value"][~valid]).all() and (cand["flags"][~valid] == 0).all()
    out, fmap, bv, ba = planning.beam_select_ref(reward, reason, n_roots, width, 1, 0.5, slots)
    assert list(fmap) == [4, 0, 5, 12, 13, 14]        # 9.0, the finished 5.0, 4.0 (3.0 and -6.0 drop) | three tied 6.0
    assert list(out["value"]) == [9.0, 5.0, 4.0, 6.0, 6.0, 6.0] and list(out["first"]) == [1, 2, 1, 2, 2, 2]
    assert list(bv) == [9.0, 6.0] and list(ba) == [1, 2]


def _before(x, y):
    """the rule written out: valid before invalid; valid by value (NaN last, ties to the lower index); invalid by index"""
    (vx, okx, ix), (vy, oky, iy) = x, y
    if okx != oky:
        return -1 if okx else 1
    if okx and np.isnan(vx) != np.isnan(vy):
        return 1 if np.isnan(vx) else -1
    if okx and not np.isnan(vx) and vx != vy:
        return -1 if vx > vy else 1
    return -1 if ix < iy else 1


def test_order_follows_the_rule_written_out():
    rng = np.random.default_rng(9)
    width, n_roots = 27, 30
    pool = np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan, 2.0, 2.0])
    cand = np.zeros(3 * width * n_roots, dtype=planning.BEAM_SLOT)
    cand["value"] = pool[rng.integers(0, len(pool), len(cand))]
    cand["flags"] = rng.integers(0, 2, len(cand))
    order = planning.beam_order(cand, n_roots)
    for i in range(n_roots):
        idx = range(i * 3 * width, (i + 1) * 3 * width)
        keys = [(cand["value"][c], bool(cand["flags"][c]), c) for c in idx]
        want = [k[2] for k in sorted(keys, key=functools.cmp_to_key(_before))]
        assert list(order[i]) == want


def test_argument_checks_need_no_device():
    w = planning.check_beam_args(10, 9, 4, 0.5)
    assert list(w) == [1.0, 0.5, 0.25, 0.125]
    for width in (0, 82, 2.0):
        with pytest.raises(ValueError):
            planning.check_beam_args(10, width, 4, 1.0)
    for horizon in (0, -1, 3.0):
        with pytest.raises(ValueError):
            planning.check_beam_args(10, 9, horizon, 1.0)
    with pytest.raises(ValueError):
        planning.check_beam_args(10, 9, 4, float("inf"))
    with pytest.raises(ValueError):
        planning.check_beam_args(10, 9, 3, 1e300)                         # gamma^2 overflows
    with pytest.raises(ValueError):
        planning.check_beam_args(2 ** 31 // 243 + 1, 81, 4, 1.0)          # 2^31 children or more
    with pytest.raises(TypeError):
        planning.BeamPlanner(object(), substeps=10)                        # not a BatchedPropagator (a sharded one, say)


def test_beam_select_refuses_bad_arguments():
    lib = _lib.load()
    vp, vq = 1 << 20, 2 << 20                                             # (never dereferenced: refused before any launch)
    ok = (vp, vp, 4, 9, 1, 1.0, vq, vp, vp, vp, vp, None)

    def call(**kw):
        names = ("reward", "reason", "n_roots", "width", "level", "weight", "d_in", "d_out", "map", "best_value", "best_action", "stream")
        args = dict(zip(names, ok))
        args.update(kw)
        return lib.bsk_beam_select(*[args[n] for n in names])

    for name in ("reward", "reason", "d_out", "map", "best_value", "best_action"):
        assert call(**{name: None}) == -1, name
    assert call(d_in=None) == -1                                          # NULL parents above level 0
    for width in (0, 82):
        assert call(width=width) == -1
    assert b"width" in lib.bsk_last_error()
    assert call(n_roots=0) == -1 and call(level=-1) == -1
    assert call(n_roots=2 ** 31 // 27 + 1) == -1
    assert b"2^31" in lib.bsk_last_error()
    for weight in (float("nan"), float("inf")):
        assert call(weight=weight) == -1
    assert call(d_in=vp) == -1
    assert b"distinct" in lib.bsk_last_error()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_beam_planner_fails_loudly_without_gpu():
    from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
    root = object.__new__(BatchedPropagator)            # (a root cannot be created here either: stand in for one)
    root.cfg, root.n_envs, root.device, root.sim_time, root.gravity_sh = default_config(4, _lib.GRAV_PM_J2), 8, 0, 0.0, None
    root._h = None
    root.stream_ptr = lambda: 0
    with pytest.raises(_lib.BskGpuUnavailable):
        planning.BeamPlanner(root, width=3, horizon=4, substeps=10)
    with pytest.raises(ValueError):
        planning.BeamPlanner(root, width=3, horizon=0, substeps=10)      # refused before any device is needed
