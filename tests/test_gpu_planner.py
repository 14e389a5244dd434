"""GPU: choosing among rollouts (bsk_select_branches) and the lookahead planner built on forks (basilisk_env_amd/planning.py).

select_branches is held bit for bit to the numpy statement of its value and choice rules (planning.branch_values / select_best,
themselves tested on the CPU).  The planner is held to an independent exhaustive search: every action sequence of every root run
through the CPU oracle (oracle.step) from the root's state and counters.  Last, plan() and the root's step on the planned actions
captured in one HIP graph replay without a copy or a synchronisation and match eager execution."""
import ctypes

import numpy as np
import pytest

from basilisk_env_amd import _hip, _lib, planning
from basilisk_env_amd._lib import FLAG_DESAT, FLAG_DRAG, FLAG_POWER, FLAG_SUN_THIRD_BODY, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from oracle import oracle

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


@pytest.mark.parametrize("gamma", [1.0, 0.99])
@pytest.mark.parametrize("group,n_groups,T", [(1, 5, 1), (3, 200, 2), (9, 700, 4), (27, 100, 5), (729, 7, 6), (100, 13, 3)])
def test_select_branches_matches_numpy_bit_for_bit(gamma, group, n_groups, T):
    rng = np.random.default_rng(group * 1000 + T)
    nb = group * n_groups
    r = rng.normal(size=(T, nb)) * 1e-2
    r[:, ::4] = np.round(r[:, ::4], 3)                 # quantised rewards: exact ties between branches
    r[:, 1::7] = 0.0
    q = ((rng.random((T, nb)) < 0.1) * rng.integers(1, 16, (T, nb))).astype(np.uint8)
    q[0, 2::11] = 1                                    # done at t = 0
    r[rng.random((T, nb)) < 0.03] = np.nan             # NaN values lose
    if n_groups > 3:
        r[:, 2 * group:3 * group] = np.nan             # a group of NaNs picks its first branch
        r[:, 3 * group:4 * group] = 0.0                # a group of exact ties picks its first branch
        q[:, 3 * group:4 * group] = 0
    first = rng.integers(0, 3, nb).astype(np.int32)
    bufs = [_upload(r), _upload(q), _upload(first), _hip.DeviceBuffer(8 * nb, 0), _hip.DeviceBuffer(8 * n_groups, 0), _hip.DeviceBuffer(4 * n_groups, 0)]
    vp = [ctypes.c_void_p(b.ptr) for b in bufs]
    _lib.check(_lib.load().bsk_select_branches(vp[0], vp[1], vp[2], T, nb, group, gamma, vp[3], vp[4], vp[5], None))
    _hip.stream_sync(0)
    values = _download(bufs[3].ptr, np.float64, nb)
    best_value = _download(bufs[4].ptr, np.float64, n_groups)
    best_action = _download(bufs[5].ptr, np.int32, n_groups)
    want_v = planning.branch_values(r, q, gamma)
    best, want_bv = planning.select_best(want_v, group)
    assert np.array_equal(values, want_v, equal_nan=True)
    assert np.array_equal(best_value, want_bv, equal_nan=True)
    assert np.array_equal(best_action, first[np.arange(n_groups) * group + best])
    if n_groups > 3:
        assert best[2] == 0 and best[3] == 0
    # the optional outputs may be NULL
    _lib.check(_lib.load().bsk_select_branches(vp[0], vp[1], vp[2], T, nb, group, gamma, None, None, vp[5], None))
    _hip.stream_sync(0)
    assert np.array_equal(_download(bufs[5].ptr, np.int32, n_groups), best_action)
    for b in bufs:
        b.free()


def _host_search(cfg, state, steps, ticks, depth, tail_steps, tail_action, k, gamma):
    """exhaustive search with the CPU oracle: every root's 3**depth sequences from tiled copies of its state and counters"""
    n = state.shape[1]
    K = 3 ** depth
    table = planning.action_table(n, depth, tail_steps, tail_action)
    st = np.ascontiguousarray(np.repeat(state, K, axis=1))
    s, t = np.repeat(steps, K).astype(np.int32), np.repeat(ticks, K).astype(np.int32)
    rew, why = [], []
    for a in table:
        _, r, _, w = oracle.step(cfg, st, s, t, a, k)
        rew.append(r)
        why.append(w)
    values = planning.branch_values(np.array(rew), np.array(why), gamma)
    return values.reshape(n, K)


@pytest.mark.parametrize("level,k", [("bare", 30), ("full", 60)])
@pytest.mark.parametrize("depth,tail", [(2, 0), (3, 2)])
def test_planner_matches_an_exhaustive_host_search(level, k, depth, tail):
    n, gamma = 32, 0.99
    cfg = default_config(4, GRAV_PM_J2)
    if level == "full":
        cfg.flags |= FLAG_POWER | FLAG_SUN_THIRD_BODY | FLAG_DRAG | FLAG_DESAT
    cfg.max_length = 6                                  # some branches end by length inside the lookahead
    root = BatchedPropagator(cfg, n)
    ic = sample_ic_batch(n, 4, seed=50 + depth)
    ic[12:16, ::9] *= 3.2                               # some wheels close to their limit: wheel terminations and penalties
    root.reset(ic)
    rng = np.random.default_rng(depth)
    for _ in range(int(rng.integers(1, 4))):
        root.step(rng.integers(0, 3, n).astype(np.int32), k)
    state = root.get_state()
    steps, ticks = root.get_counters()
    planner = planning.LookaheadPlanner(root, depth=depth, tail_steps=tail, tail_action=1, gamma=gamma, substeps=k)
    actions, values = planner.plan_host()
    host = _host_search(cfg, state, steps, ticks, depth, tail, 1, k, gamma)
    best, best_v = planning.select_best(host.ravel(), 3 ** depth)
    srt = np.sort(host, axis=1)
    near = (srt[:, -1] != srt[:, -2]) & (np.abs(srt[:, -1] - srt[:, -2]) <= 1e-9 * np.abs(srt[:, -1]))
    print("near-ties skipped: %d of %d roots" % (int(near.sum()), n))
    ok = ~near
    assert ok.sum() >= n // 2
    assert np.array_equal(actions[ok], (best % 3)[ok])
    assert np.allclose(values, best_v, rtol=1e-11, atol=0.0)
    # every branch value too, and the root itself untouched by planning
    assert np.allclose(planner.last_branch_values(), host, rtol=1e-11, atol=1e-300)
    assert np.array_equal(root.get_state(), state)
    planner.close()
    root.close()


def test_planned_steps_replay_from_one_graph():
    import torch
    n, k, depth = 64, 10, 2
    cfg = default_config(4, GRAV_PM_J2)
    cfg.max_length = 1000
    side = torch.cuda.Stream()
    ic = sample_ic_batch(n, 4, seed=77)
    with torch.cuda.stream(side):
        g_root = BatchedPropagator(cfg, n, stream=side.cuda_stream)
        e_root = BatchedPropagator(cfg, n, stream=side.cuda_stream)
        for p in (g_root, e_root):
            p.reset(ic)
        g_plan = planning.LookaheadPlanner(g_root, depth=depth, substeps=k)
        e_plan = planning.LookaheadPlanner(e_root, depth=depth, substeps=k)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            view = g_plan.plan()
            g_root.step_device(view.__cuda_array_interface__["data"][0], k)
        c0 = BatchedPropagator.debug_counters()
        for _ in range(3):
            graph.replay()
        assert BatchedPropagator.debug_counters() == c0
        torch.cuda.synchronize()
        taken = []
        for _ in range(3):
            ev = e_plan.plan()
            acts = torch.from_dlpack(ev)                         # zero-copy view of the planner's buffer
            assert acts.data_ptr() == ev.__cuda_array_interface__["data"][0]
            taken.append(acts.cpu().numpy().copy())
            e_root.step_device(acts.data_ptr(), k)
        torch.cuda.synchronize()
        assert np.array_equal(g_plan.last_actions(), taken[-1])
        assert np.array_equal(g_root.get_state(), e_root.get_state())
        for a, b in zip(g_root.get_obs(), e_root.get_obs()):
            assert np.array_equal(a, b)
        assert np.array_equal(g_root.get_counters()[1], np.full(n, 3 * k))
        del graph
        for x in (g_plan, e_plan, g_root, e_root):
            x.close()
