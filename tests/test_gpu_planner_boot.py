"""GPU: planning with a learned value at the leaves (include/bskgpu.h: bsk_policy_value, bsk_select_branches_boot,
bsk_beam_select_boot; basilisk_env_amd/planning.py: LookaheadPlanner / BeamPlanner with a value_policy).

bsk_policy_value is held bit for bit to bsk_policy_act's d_value (both activations) and, for relu, to policy_ref.mlp_ref.  The two
selection kernels are held bit for bit to their numpy statements (planning.branch_values_boot / beam_select_boot_ref, themselves
held to a branch-by-branch loop on the CPU).  The planners are held to those statements on their own histories, to each other
where the beam keeps every sequence, and - without a value policy - to what they gave before.  Last: capture into one HIP graph,
and the value targets of planning.distill on a bootstrapped planner."""
import ctypes

import numpy as np
import pytest

from _device_bits import bits as _bits, same as _same
from _policy_bounds import observation_like, seeded_policy
from basilisk_env_amd import _hip, _lib, planning
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch

pytestmark = pytest.mark.gpu


def _upload(a):
    a = np.ascontiguousarray(a)
    b = _hip.DeviceBuffer(max(a.nbytes, 1), 0)
    _hip.check(_hip.runtime().hipMemcpyAsync(ctypes.c_void_p(b.ptr), ctypes.c_void_p(a.ctypes.data), a.nbytes, _hip.hipMemcpyHostToDevice,
                                             ctypes.c_void_p(0)), "hipMemcpyAsync")
    _hip.stream_sync(0)
    return b


def _download(ptr, dtype, count):
    out = np.empty(count, dtype=dtype)
    _hip.check(_hip.runtime().hipMemcpyAsync(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), out.nbytes, _hip.hipMemcpyDeviceToHost,
                                             ctypes.c_void_p(0)), "hipMemcpyAsync")
    _hip.stream_sync(0)
    return out


def _same_values(a, b):
    """equal bit for bit where they are numbers - the sign of zero included - and NaN where NaN: WHICH NaN an invalid operation
    such as 0 * inf makes is the hardware's choice (x86 sets the sign bit, gfx950 does not), so NaN bits are not compared"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(_bits(a)[~nan], _bits(b)[~nan])


# --------------------------------------------------------------------------------------------------------------- bsk_policy_value
# (action network, value network): every depth of the value network, and an action network narrower and wider than it - the LDS
# columns are sized by the wider of the two
VALUE_NETS = {"v0_a16": ((16,), ()), "v16_a128": ((128,), (16,)), "v64x2_a16": ((16,), (64, 64)), "v128x3_a32x2": ((32, 32), (128, 128, 128))}
CANARY = np.float32(-1234.5)


@pytest.mark.parametrize("activation", ["relu", "tanh"])
@pytest.mark.parametrize("net", sorted(VALUE_NETS))
def test_policy_value_equals_the_value_of_policy_act_bit_for_bit(net, activation):
    hidden, value_hidden = VALUE_NETS[net]
    spec, params = seeded_policy(hidden, activation, value_hidden, seed=40 + len(value_hidden))
    pol = P.DevicePolicy(spec, params)
    lib = _lib.load()
    for n in (1, 63, 64, 65, 200):
        stride = n + 9                                                    # obs_stride > n: the columns beyond n are not the batch's
        obs = observation_like(stride, seed=n)
        d_obs = _upload(obs)
        d_out = _upload(np.full(n + 64, CANARY, np.float32))
        _lib.check(lib.bsk_policy_value(pol._handle(), ctypes.c_void_p(d_obs.ptr), stride, n, ctypes.c_void_p(d_out.ptr), None))
        _hip.stream_sync(0)
        got = _download(d_out.ptr, np.float32, n + 64)
        assert _same(got[n:], np.full(64, CANARY, np.float32)), (net, n)          # nothing beyond d_value[n - 1] is written
        act = pol.enqueue(d_obs.ptr, stride, n, "greedy", ("value",))
        _hip.stream_sync(0)
        want = _download(act["value"].ptr, np.float32, n)
        assert _same(got[:n], want), (net, activation, n)
        assert np.isfinite(want).all() and (n < 8 or len(set(want.tolist())) > 1)
        if activation == "relu":
            assert _same(got[:n], P.mlp_ref(spec, params, obs[:, :n])[1]), (net, n)
        # the binding makes the same call
        d_out2 = _upload(np.full(n + 64, CANARY, np.float32))
        pol.value_enqueue(d_obs.ptr, stride, n, d_out2.ptr)
        _hip.stream_sync(0)
        assert _same(_download(d_out2.ptr, np.float32, n + 64), got)
        for b in (d_obs, d_out, d_out2):
            b.free()
    pol.close()


def test_policy_value_leaves_the_draw_counter_alone_and_refuses_bad_arguments():
    spec, params = seeded_policy((16,), "relu", (16,), seed=3)
    pol = P.DevicePolicy(spec, params)
    pol.set_rng(11, 5)
    lib, vp = _lib.load(), ctypes.c_void_p
    d_obs, d_out = _upload(observation_like(80, seed=1)), _upload(np.zeros(80, np.float32))
    pol.value_enqueue(d_obs.ptr, 80, 70, d_out.ptr)
    assert pol.get_rng() == (11, 5)
    h = pol._handle()
    assert lib.bsk_policy_value(h, None, 80, 70, vp(d_out.ptr), None) == -1
    assert lib.bsk_policy_value(h, vp(d_obs.ptr), 80, 70, None, None) == -1
    assert lib.bsk_policy_value(None, vp(d_obs.ptr), 80, 70, vp(d_out.ptr), None) == -1
    assert lib.bsk_policy_value(h, vp(d_obs.ptr), 80, 0, vp(d_out.ptr), None) == -1
    assert lib.bsk_policy_value(h, vp(d_obs.ptr), 80, -3, vp(d_out.ptr), None) == -1
    assert lib.bsk_policy_value(h, vp(d_obs.ptr), 69, 70, vp(d_out.ptr), None) == -1
    assert b"obs_stride" in lib.bsk_last_error()
    bare_spec, bare_params = seeded_policy((16,), "relu", seed=3)
    bare = P.DevicePolicy(bare_spec, bare_params)
    assert lib.bsk_policy_value(bare._handle(), vp(d_obs.ptr), 80, 70, vp(d_out.ptr), None) == -1
    assert b"no value network" in lib.bsk_last_error()
    with pytest.raises(_lib.BskError):
        bare.value_enqueue(d_obs.ptr, 80, 70, d_out.ptr)
    root = BatchedPropagator(default_config(3, GRAV_PM_J2), 5)
    with pytest.raises(ValueError, match="no value network"):
        planning.LookaheadPlanner(root, depth=1, substeps=10, value_policy=bare)
    with pytest.raises(ValueError, match="no value network"):
        planning.BeamPlanner(root, width=3, horizon=2, substeps=10, value_policy=bare)
    for x in (root, bare, pol):
        x.close()
    d_obs.free()
    d_out.free()


# ------------------------------------------------------------------------------------------------------- bsk_select_branches_boot
def _histories(group, n_groups, T):
    """the adversarial contents of tests/test_gpu_planner.py, plus the leaf's own"""
    rng = np.random.default_rng(group * 1000 + T)
    nb = group * n_groups
    r = rng.normal(size=(T, nb)) * 1e-2
    r[:, ::4] = np.round(r[:, ::4], 3)                 # quantised rewards: exact ties between branches
    r[:, 1::7] = 0.0
    q = ((rng.random((T, nb)) < 0.1) * rng.integers(1, 16, (T, nb))).astype(np.uint8)
    q[0, 2::11] = 1                                    # an end at t = 0
    q[:T - 1, 3::11] = 0
    q[T - 1, 3::11] = 2                                # an end at t = T - 1 and not before: no bootstrap
    r[rng.random((T, nb)) < 0.03] = np.nan             # NaN values lose
    leaf = np.round(rng.normal(size=nb) * 1e-2, 3).astype(np.float32)       # quantised like the rewards: ties survive the leaf term
    leaf[rng.random(nb) < 0.05] = np.nan               # a NaN leaf makes the branch lose
    leaf[rng.random(nb) < 0.05] = -np.inf
    if n_groups > 3:
        r[:, 2 * group:3 * group] = np.nan             # a group of NaNs picks its first branch
        r[:, 3 * group:4 * group] = 0.0                # a group of exact ties picks its first branch
        q[:, 3 * group:4 * group] = 0
        leaf[3 * group:4 * group] = 0.25
    first = rng.integers(0, 3, nb).astype(np.int32)
    return r, q, leaf, first


def _run_select(r, q, first, T, nb, group, gamma, leaf):
    n_groups = nb // group
    bufs = [_upload(r), _upload(q), _upload(first), _hip.DeviceBuffer(8 * nb, 0), _hip.DeviceBuffer(8 * n_groups, 0),
            _hip.DeviceBuffer(4 * n_groups, 0)] + ([] if leaf is None else [_upload(leaf)])
    vp = [ctypes.c_void_p(b.ptr) for b in bufs]
    lib = _lib.load()
    if leaf is None:
        _lib.check(lib.bsk_select_branches(vp[0], vp[1], vp[2], T, nb, group, gamma, vp[3], vp[4], vp[5], None))
    else:
        _lib.check(lib.bsk_select_branches_boot(vp[0], vp[1], vp[2], T, nb, group, gamma, vp[6], vp[3], vp[4], vp[5], None))
    _hip.stream_sync(0)
    out = (_download(bufs[3].ptr, np.float64, nb), _download(bufs[4].ptr, np.float64, n_groups), _download(bufs[5].ptr, np.int32, n_groups))
    if leaf is not None:                               # the optional outputs may be NULL
        _lib.check(lib.bsk_select_branches_boot(vp[0], vp[1], vp[2], T, nb, group, gamma, vp[6], None, None, vp[5], None))
        _hip.stream_sync(0)
        assert np.array_equal(_download(bufs[5].ptr, np.int32, n_groups), out[2])
    for b in bufs:
        b.free()
    return out


@pytest.mark.parametrize("gamma", [1.0, 0.99, 0.0])
@pytest.mark.parametrize("group,n_groups,T", [(1, 5, 1), (3, 50, 2), (64, 3, 3), (65, 3, 3), (243, 2, 5)])
def test_select_branches_boot_matches_numpy_bit_for_bit(gamma, group, n_groups, T):
    r, q, leaf, first = _histories(group, n_groups, T)
    nb = group * n_groups
    values, best_value, best_action = _run_select(r, q, first, T, nb, group, gamma, leaf)
    want_v = planning.branch_values_boot(r, q, gamma, leaf)
    best, want_bv = planning.select_best(want_v, group)
    assert _same_values(values, want_v)
    assert np.array_equal(best_value, want_bv, equal_nan=True)
    assert np.array_equal(best_action, first[np.arange(n_groups) * group + best])
    ended = (q != 0).any(axis=0)
    plain = planning.branch_values(r, q, gamma)
    assert np.array_equal(values[ended], plain[ended], equal_nan=True)           # an ended branch takes no leaf term ...
    if group >= 3:                                                                 # (branch 3 lies outside the NaN and tie groups)
        assert ended[3] and not (q[:T - 1, 3] != 0).any()                         # ... the one that ended at the last step too
    if n_groups > 3:
        assert best[2] == 0 and best[3] == 0
    # with an all-zero leaf the kernel gives what bsk_select_branches gives
    zero = _run_select(r, q, first, T, nb, group, gamma, np.zeros(nb, np.float32))
    old = _run_select(r, q, first, T, nb, group, gamma, None)
    for a, b in zip(zero, old):
        assert np.array_equal(a, b, equal_nan=True)


# ----------------------------------------------------------------------------------------------------------- bsk_beam_select_boot
def _random_level(rng, n_roots, width):
    n = 3 * width * n_roots
    r = rng.normal(size=n) * 1e-2
    r[::3] = np.round(r[::3], 3)                       # quantised rewards: exact ties between candidates
    r[1::5] = 0.0
    r[rng.random(n) < 0.03] = np.nan                   # NaN values after every number
    q = ((rng.random(n) < 0.2) * rng.integers(1, 16, n)).astype(np.uint8)
    slots = np.zeros(n_roots * width, dtype=planning.BEAM_SLOT)
    slots["value"] = np.round(rng.normal(size=len(slots)), 2)
    slots["value"][rng.random(len(slots)) < 0.03] = np.nan
    slots["first"] = rng.integers(0, 3, len(slots))
    slots["flags"] = rng.choice([0, planning.BEAM_VALID, planning.BEAM_VALID | planning.BEAM_LIVE, planning.BEAM_LIVE], len(slots),
                                p=[0.1, 0.2, 0.6, 0.1])                     # invalid, finished and live parents
    leaf = np.round(rng.normal(size=n), 2).astype(np.float32)               # of the size of the parents' values: the order changes
    leaf[::13] = 0.0
    leaf[rng.random(n) < 0.03] = np.nan
    leaf[rng.random(n) < 0.02] = -np.inf
    return r, q, slots, leaf


def _run_beam(r, q, slots, leaf, n_roots, width, level, weight, boot_weight, with_key=True):
    ns = n_roots * width
    bufs = [_upload(r), _upload(q), _upload(slots), _hip.DeviceBuffer(16 * ns, 0), _hip.DeviceBuffer(4 * ns, 0),
            _hip.DeviceBuffer(8 * n_roots, 0), _hip.DeviceBuffer(4 * n_roots, 0), _upload(np.full(ns, -7.0)),
            _upload(np.zeros(1, np.float32) if leaf is None else leaf)]
    vp = [ctypes.c_void_p(b.ptr) for b in bufs]
    d_in = vp[2] if level else None
    lib = _lib.load()
    if leaf is None:
        _lib.check(lib.bsk_beam_select(vp[0], vp[1], n_roots, width, level, weight, d_in, vp[3], vp[4], vp[5], vp[6], None))
    else:
        _lib.check(lib.bsk_beam_select_boot(vp[0], vp[1], n_roots, width, level, weight, boot_weight, vp[8], d_in, vp[3], vp[4],
                                            vp[7] if with_key else None, vp[5], vp[6], None))
    _hip.stream_sync(0)
    out = (_download(bufs[3].ptr, planning.BEAM_SLOT, ns), _download(bufs[4].ptr, np.int32, ns), _download(bufs[7].ptr, np.float64, ns),
           _download(bufs[5].ptr, np.float64, n_roots), _download(bufs[6].ptr, np.int32, n_roots))
    for b in bufs:
        b.free()
    return out


@pytest.mark.parametrize("width", [1, 3, 9, 28, 81])
def test_beam_select_boot_matches_numpy_bit_for_bit(width):
    rng = np.random.default_rng(500 + width)
    per = 256 // (3 * width)                           # roots per workgroup (width 28: three, and four idle threads)
    n_roots = 2 * per + 1                              # not a multiple of it: the last workgroup is part empty
    differs = 0
    for level, gamma in ((0, 1.0), (2, 0.99)):
        w = planning.level_weights(gamma, level + 2)
        weight, boot_weight = float(w[level]), float(w[level + 1])
        r, q, slots, leaf = _random_level(rng, n_roots, width)
        got = _run_beam(r, q, slots, leaf, n_roots, width, level, weight, boot_weight)
        want = planning.beam_select_boot_ref(r, q, leaf, n_roots, width, level, weight, boot_weight, slots if level else None)
        what = "width %d, %d roots, level %d" % (width, n_roots, level)
        assert _same_values(got[0]["value"], want[0]["value"]), what
        assert np.array_equal(got[0]["first"], want[0]["first"]) and np.array_equal(got[0]["flags"], want[0]["flags"]), what
        assert np.array_equal(got[1], want[1]), what
        for k in (2, 3):
            assert np.array_equal(got[k], want[k], equal_nan=True), what
        assert np.array_equal(got[4], want[4]), what
        # the slots hold the un-bootstrapped values: those of bsk_beam_select's candidates
        cand = planning.beam_candidates(r, q, n_roots, width, level, weight, slots if level else None)
        kept = got[1] >= 0
        assert np.array_equal(got[0]["value"][kept], cand["value"][got[1][kept]], equal_nan=True), what
        # d_key = NULL is accepted and changes nothing else
        nokey = _run_beam(r, q, slots, leaf, n_roots, width, level, weight, boot_weight, with_key=False)
        assert nokey[0].tobytes() == got[0].tobytes() and np.array_equal(nokey[1], got[1]) and (nokey[2] == -7.0).all()
        assert np.array_equal(nokey[3], got[3], equal_nan=True) and np.array_equal(nokey[4], got[4])
        # against bsk_beam_select on the same level: with the leaf the kept set (or its order) is another one
        plain = _run_beam(r, q, slots, None, n_roots, width, level, weight, 0.0)
        ref_plain = planning.beam_select_ref(r, q, n_roots, width, level, weight, slots if level else None)
        assert np.array_equal(plain[1], ref_plain[1]), what
        differs += int(not np.array_equal(plain[1], got[1]))
        if level and width in (3, 9, 28):
            assert set(plain[1][kept].tolist()) != set(got[1][kept].tolist()), what       # a kept SET that differs, not only its order
    assert differs == 2


# ------------------------------------------------------------------------------------------------------------------ the planners
K = 10


def _small_root(stream=None, n=5, seed=33, max_length=5):
    """bare J2, 3 wheels; step counters staggered by hand so that within a lookahead of 2 or 3 env steps some roots end by length
    at the first step, some at the last, and some not at all"""
    cfg = default_config(3, GRAV_PM_J2)
    cfg.max_length = max_length
    root = BatchedPropagator(cfg, n) if stream is None else BatchedPropagator(cfg, n, stream=stream)
    root.reset(sample_ic_batch(n, 3, seed=seed))
    root.step(np.zeros(n, np.int32), K)
    steps, ticks = root.get_counters()
    root.set_counters(steps + np.arange(n, dtype=np.int32) % 5, ticks)
    return root


def _planner_histories(planner):
    T, nb = planner.n_steps, planner.n_branch
    r = planner._read(planner.d_reward_hist, np.float64, T * nb).reshape(T, nb)
    q = planner._read(planner.d_reason_hist, np.uint8, T * nb).reshape(T, nb)
    return r, q


@pytest.fixture(scope="module")
def value_policy():
    spec, params = seeded_policy((16,), "relu", (16,), seed=21)
    pol = P.DevicePolicy(spec, params)
    yield spec, params, pol
    pol.close()


def test_lookahead_planner_bootstraps_its_own_histories(value_policy):
    spec, params, pol = value_policy
    gamma = 0.97
    root = _small_root()
    state = root.get_state()
    planner = planning.LookaheadPlanner(root, depth=2, tail_steps=1, gamma=gamma, substeps=K, value_policy=pol)
    actions, values = planner.plan_host()
    r, q = _planner_histories(planner)
    leaf = P.mlp_ref(spec, params, planner.branch.get_obs()[0])[1]
    assert leaf.shape == (planner.n_branch,) and leaf.dtype == np.float32
    assert _same(_download(planner.d_leaf.ptr, np.float32, planner.n_branch), leaf)
    want = planning.branch_values_boot(r, q, gamma, leaf)
    assert _same_values(planner.last_branch_values().ravel(), want)
    best, best_v = planning.select_best(want, 9)
    assert np.array_equal(values, best_v) and np.array_equal(actions, (best % 3).astype(np.int32))
    ended = (q != 0).any(axis=0)
    last_only = (q[-1] != 0) & ~(q[:-1] != 0).any(axis=0)
    assert (q[0] != 0).any() and last_only.any() and (~ended).any()             # ends at the first step, at the last alone, and none
    plain = planning.branch_values(r, q, gamma)
    assert np.array_equal(want[ended], plain[ended]) and (want[~ended] != plain[~ended]).any()
    assert np.array_equal(root.get_state(), state)                              # planning leaves the root untouched
    planner.close()
    root.close()


@pytest.mark.parametrize("bootstrap", ["every", "last"])
def test_full_width_beam_equals_the_bootstrapped_lookahead(value_policy, bootstrap):
    spec, params, pol = value_policy
    gamma = 0.97
    root = _small_root()
    look = planning.LookaheadPlanner(root, depth=2, gamma=gamma, substeps=K, value_policy=pol)
    beam = planning.BeamPlanner(root, width=9, horizon=2, gamma=gamma, substeps=K, value_policy=pol, bootstrap=bootstrap)
    _, want = look.plan_host()
    actions, values = beam.plan_host()
    assert _same_values(values, want)
    branch = look.last_branch_values()
    for i in range(root.n_envs):
        assert actions[i] in set(np.flatnonzero(branch[i] == want[i]) % 3)
    # the keys are the lookahead's branch values in rank order, the slots keep the un-bootstrapped returns (a sequence that ended
    # at the first step is three branches there and one slot here: compared as sets)
    keys, vals = beam.last_beam_keys(), beam.last_beam_values()
    assert np.array_equal(keys[:, 0], values)
    r, q = _planner_histories(look)
    plain = planning.branch_values(r, q, gamma).reshape(root.n_envs, 9)
    assert (q[0] != 0).any() and ((q[-1] != 0) & (q[0] == 0)).any() and (q == 0).all(axis=0).any()
    moved = 0
    for i in range(root.n_envs):
        kept = ~np.isnan(keys[i])
        assert np.array_equal(np.isnan(vals[i]), ~kept) and kept[0]
        assert (np.diff(keys[i][kept]) <= 0).all()
        assert np.array_equal(np.unique(keys[i][kept]), np.unique(branch[i]))
        assert np.array_equal(np.unique(vals[i][kept]), np.unique(plain[i]))
        moved += int((vals[i][kept] != keys[i][kept]).sum())
    assert moved > 0
    for x in (look, beam, root):
        x.close()


def test_without_a_value_policy_the_planners_give_what_they_gave():
    gamma = 0.97
    root = _small_root()
    look = planning.LookaheadPlanner(root, depth=2, tail_steps=1, gamma=gamma, substeps=K)
    look2 = planning.LookaheadPlanner(root, depth=2, gamma=gamma, substeps=K, value_policy=None)
    beam = planning.BeamPlanner(root, width=9, horizon=2, gamma=gamma, substeps=K, value_policy=None, bootstrap="last")
    for p in (look, look2, beam):
        assert p.value_policy is None and not hasattr(p, "d_leaf") and not hasattr(p, "d_keys")       # nothing more is allocated
    actions, values = look.plan_host()
    r, q = _planner_histories(look)
    want = planning.branch_values(r, q, gamma)                                  # bsk_select_branches' statement, no leaf term
    assert _same_values(look.last_branch_values().ravel(), want)
    best, best_v = planning.select_best(want, 9)
    assert np.array_equal(values, best_v) and np.array_equal(actions, (best % 3).astype(np.int32))
    _, v2 = look2.plan_host()
    r2, q2 = _planner_histories(look2)
    assert np.array_equal(v2, planning.select_best(planning.branch_values(r2, q2, gamma), 9)[1])
    _, vb = beam.plan_host()
    assert _same_values(vb, v2)
    assert np.array_equal(beam.last_beam_values()[:, 0], vb)
    with pytest.raises(ValueError):
        beam.last_beam_keys()
    for x in (look, look2, beam, root):
        x.close()


@pytest.mark.parametrize("kind", ["lookahead", "beam"])
def test_bootstrapped_plans_replay_from_one_graph(value_policy, kind):
    import torch
    spec, params, pol = value_policy
    side = torch.cuda.Stream()

    def make(root):
        if kind == "beam":
            return planning.BeamPlanner(root, width=3, horizon=3, gamma=0.97, substeps=K, value_policy=pol)
        return planning.LookaheadPlanner(root, depth=2, tail_steps=1, gamma=0.97, substeps=K, value_policy=pol)

    with torch.cuda.stream(side):
        g_root, e_root = (_small_root(side.cuda_stream, n=64, max_length=1000) for _ in range(2))
        g_plan, e_plan = make(g_root), make(e_root)
        torch.cuda.synchronize()
        c0 = BatchedPropagator.debug_counters()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):             # capturable from the first call: nothing was planned before
            view = g_plan.plan()
            g_root.step_device(view.__cuda_array_interface__["data"][0], K)
        for _ in range(3):
            graph.replay()
        ev = None
        for _ in range(3):
            ev = e_plan.plan()
            e_root.step_device(ev.__cuda_array_interface__["data"][0], K)
        assert BatchedPropagator.debug_counters() == c0       # capture, replays and eager plans: no copy, no synchronisation
        torch.cuda.synchronize()
        assert np.array_equal(g_plan.last_actions(), e_plan.last_actions())
        assert _same_values(g_plan.last_values(), e_plan.last_values())
        assert _same(_download(g_plan.d_leaf.ptr, np.float32, 64), _download(e_plan.d_leaf.ptr, np.float32, 64))
        if kind == "beam":
            assert np.array_equal(g_plan.last_beam_keys(), e_plan.last_beam_keys(), equal_nan=True)
            assert np.array_equal(g_plan.last_beam_values(), e_plan.last_beam_values(), equal_nan=True)
        assert np.array_equal(g_root.get_state(), e_root.get_state())
        for a, b in zip(g_root.get_obs(), e_root.get_obs()):
            assert np.array_equal(a, b)
        del graph
        for x in (g_plan, e_plan, g_root, e_root):
            x.close()


def test_distill_fits_the_value_network_to_bootstrapped_targets():
    """One step of planning.distill on a planner that reads the value network being fitted.  For relu networks the value is the
    restatement's bit for bit, so the value-loss column EQUALS policy_ref.fit_stats_ref's on the planner's bootstrapped
    d_best_value (the rule of tests/test_gpu_fit.py: _check_stats) - no tolerance is involved."""
    import torch
    n, gamma = 64, 0.97
    spec, params = seeded_policy((16,), "relu", (16,), seed=16)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        root = _small_root(side.cuda_stream, n=n, max_length=1000)
        pol = P.DevicePolicy(spec, params)
        fit = P.PolicyFit(pol, lr=1e-2)
        planner = planning.LookaheadPlanner(root, depth=1, gamma=gamma, substeps=K, value_policy=pol)
        obs0 = root.get_obs()[0]
        rows = planning.distill(planner, pol, fit, root, n_steps=1, value_targets=True)
        targets, labels = planner.last_values(), planner.last_actions()          # what the one plan left on the device
        # the targets are n-step returns through the planner's own max, formed with the parameters of BEFORE the fit's step
        r, q = _planner_histories(planner)
        leaf = P.mlp_ref(spec, params, planner.branch.get_obs()[0])[1]
        best, want_targets = planning.select_best(planning.branch_values_boot(r, q, gamma, leaf), 3)
        assert _same_values(targets, want_targets) and np.array_equal(labels, (best % 3).astype(np.int32))
        plain = planning.select_best(planning.branch_values(r, q, gamma), 3)[1]
        assert (targets != plain).all()                                           # (no episode ends this early: every target has a leaf term)
        ref = P.fit_stats_ref(spec, params, obs0, labels, None, targets)
        print("value_loss_sum: device %.17g, numpy %.17g" % (rows[0, 1], ref[1]))
        assert rows.shape == (1, 4) and rows[0, 3] == n == ref[3]
        assert _same(np.float64(rows[0, 1]), np.float64(ref[1])) and ref[1] > 0
        assert rows[0, 2] == ref[2]
        st = fit.state()
        a_end = 10 + sum(o * i + o for o, i in P.layer_shapes(spec)[0])
        assert st["steps"] == 1 and not np.array_equal(st["theta"][a_end:], params[a_end:].astype(np.float64))    # the value network moved
        for x in (fit, planner, pol, root):
            x.close()
