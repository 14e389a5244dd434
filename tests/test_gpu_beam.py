"""GPU: one beam level (bsk_beam_select) and the beam planner built on it (basilisk_env_amd/planning.py: BeamPlanner).

bsk_beam_select is held bit for bit to its numpy statement (planning.beam_select_ref, itself held on the CPU to an exhaustive
search and a greedy walk).  The planner is held to LookaheadPlanner where the beam is wide enough to keep every sequence, to a
replay of its own best sequences through bsk_step_n and bsk_select_branches, and to a host beam search over the CPU oracle.
Last, plan() and the root's step on the planned actions captured in one HIP graph replay without a copy or a synchronisation
and match eager execution."""
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
    return r, q, slots


@pytest.mark.parametrize("width", [1, 2, 3, 8, 9, 27, 64, 81])
def test_beam_select_matches_numpy_bit_for_bit(width):
    rng = np.random.default_rng(width)
    big = 65536 // (3 * width) + 7                     # more than 65 536 candidates
    for n_roots in (1, 5, big):
        for level, gamma in ((0, 1.0), (1, 1.0), (3, 0.99), (5, 0.99)):
            weight = float(planning.level_weights(gamma, level + 1)[level])
            r, q, slots = _random_level(rng, n_roots, width)
            ns = n_roots * width
            bufs = [_upload(r), _upload(q), _upload(slots), _hip.DeviceBuffer(16 * ns, 0), _hip.DeviceBuffer(4 * ns, 0),
                    _hip.DeviceBuffer(8 * n_roots, 0), _hip.DeviceBuffer(4 * n_roots, 0)]
            vp = [ctypes.c_void_p(b.ptr) for b in bufs]
            d_in = vp[2] if level else None
            _lib.check(_lib.load().bsk_beam_select(vp[0], vp[1], n_roots, width, level, weight, d_in, vp[3], vp[4], vp[5], vp[6], None))
            _hip.stream_sync(0)
            out = _download(bufs[3].ptr, planning.BEAM_SLOT, ns)
            got = (out, _download(bufs[4].ptr, np.int32, ns), _download(bufs[5].ptr, np.float64, n_roots),
                   _download(bufs[6].ptr, np.int32, n_roots))
            want = planning.beam_select_ref(r, q, n_roots, width, level, weight, slots if level else None)
            what = "width %d, %d roots, level %d" % (width, n_roots, level)
            assert np.array_equal(got[0]["value"], want[0]["value"], equal_nan=True), what
            assert np.array_equal(got[0]["first"], want[0]["first"]), what
            assert np.array_equal(got[0]["flags"], want[0]["flags"]), what
            for k in (1, 2, 3):
                assert np.array_equal(got[k], want[k], equal_nan=True), what
            for b in bufs:
                b.free()


def _root(level, n, seed, max_length):
    cfg = default_config(4, GRAV_PM_J2)
    if level == "full":
        cfg.flags |= FLAG_POWER | FLAG_SUN_THIRD_BODY | FLAG_DRAG | FLAG_DESAT
    cfg.max_length = max_length                         # some sequences end by length inside the search
    root = BatchedPropagator(cfg, n)
    ic = sample_ic_batch(n, 4, seed=seed)
    ic[12:16, ::9] *= 3.2                               # some wheels close to their limit: wheel terminations and penalties
    root.reset(ic)
    return cfg, root


def _advance(root, k, seed):
    rng = np.random.default_rng(seed)
    for _ in range(int(rng.integers(1, 4))):
        root.step(rng.integers(0, 3, root.n_envs).astype(np.int32), k)


@pytest.mark.parametrize("level,k", [("bare", 30), ("full", 60)])
@pytest.mark.parametrize("depth", [2, 3, 4])
def test_full_width_beam_equals_the_lookahead_planner(level, k, depth):
    n, gamma = 32, 0.99
    cfg, root = _root(level, n, 80 + depth, max_length=6)
    _advance(root, k, depth)
    state, (steps, ticks), obs = root.get_state(), root.get_counters(), root.get_obs()
    look = planning.LookaheadPlanner(root, depth=depth, gamma=gamma, substeps=k)
    beam = planning.BeamPlanner(root, width=3 ** depth, horizon=depth, gamma=gamma, substeps=k)
    _, want = look.plan_host()
    actions, values = beam.plan_host()
    assert np.array_equal(values, want)
    branch = look.last_branch_values()
    for i in range(n):
        assert actions[i] in set(np.flatnonzero(branch[i] == want[i]) % 3)
    # planning leaves the root untouched
    assert np.array_equal(root.get_state(), state)
    assert all(np.array_equal(a, b) for a, b in zip(root.get_counters(), (steps, ticks)))
    assert all(np.array_equal(a, b) for a, b in zip(root.get_obs(), obs))
    look.close()
    beam.close()
    root.close()


def test_best_sequences_replay_to_the_planned_values():
    n, k, width, H, gamma = 32, 60, 4, 12, 0.99
    cfg, root = _root("full", n, 91, max_length=10)
    _advance(root, k, 91)
    beam = planning.BeamPlanner(root, width=width, horizon=H, gamma=gamma, substeps=k)
    actions, values = beam.plan_host()
    seq = beam.last_sequences()
    best = seq[:, 0, :]
    assert (best >= 0).all() and np.array_equal(best[:, 0], actions)
    assert (seq < 0).any(axis=2).sum() == np.isnan(beam.last_beam_values()).sum()      # (empty slots read -1 and NaN alike)
    replay = BatchedPropagator(cfg, n)
    replay.fork_from(root, np.arange(n))
    _, rew, why = replay.rollout(H, k, actions=best.T)
    bufs = [_upload(rew), _upload(why), _upload(best[:, 0].copy()), _hip.DeviceBuffer(8 * n, 0), _hip.DeviceBuffer(4 * n, 0)]
    vp = [ctypes.c_void_p(b.ptr) for b in bufs]
    _lib.check(_lib.load().bsk_select_branches(vp[0], vp[1], vp[2], H, n, 1, gamma, None, vp[3], vp[4], None))
    _hip.stream_sync(0)
    assert np.array_equal(_download(bufs[3].ptr, np.float64, n), values)
    assert np.array_equal(_download(bufs[4].ptr, np.int32, n), actions)
    assert (why != 0).any()                              # (some replayed sequences end inside the horizon)
    for b in bufs:
        b.free()
    for x in (beam, replay, root):
        x.close()


def _host_beam(cfg, state, steps, ticks, n, width, H, k, weights):
    """the beam search on the CPU oracle: slot and child states forked by numpy indexing, each level chosen by beam_select_ref.
    -> (final slots, best actions, roots with a near-tie at a kept / dropped boundary or between ranks 0 and 1 of any level)"""
    ns = n * width
    c = np.arange(3 * ns)
    st = np.ascontiguousarray(np.repeat(state, width, axis=1))
    s, t = np.repeat(steps, width).astype(np.int32), np.repeat(ticks, width).astype(np.int32)
    slots, near = None, np.zeros(n, dtype=bool)
    for lv in range(H):
        cst, cs, ct = np.ascontiguousarray(st[:, c // 3]), s[c // 3].copy(), t[c // 3].copy()
        _, r, _, q = oracle.step(cfg, cst, cs, ct, (c % 3).astype(np.int32), k)
        cand = planning.beam_candidates(r, q, n, width, lv, weights[lv], slots)
        order = planning.beam_order(cand, n)
        v, ok = cand["value"][order], (cand["flags"][order] & planning.BEAM_VALID) != 0
        for i, j in ((0, 1), (width - 1, width)):
            gap = np.abs(v[:, i] - v[:, j])
            near |= ok[:, i] & ok[:, j] & (gap != 0) & (gap <= 1e-9 * np.abs(v[:, i]))
        slots, fmap, _, best_action = planning.beam_select_ref(r, q, n, width, lv, weights[lv], slots)
        sel = fmap >= 0
        st[:, sel], s[sel], t[sel] = cst[:, fmap[sel]], cs[fmap[sel]], ct[fmap[sel]]
    return slots, best_action, near


@pytest.mark.parametrize("level,k,width,H", [("bare", 30, 4, 8), ("full", 60, 3, 6)])
def test_beam_planner_matches_a_host_beam_search_on_the_oracle(level, k, width, H):
    n, gamma = 32, 0.99
    cfg, root = _root(level, n, 60 + H, max_length=9)
    _advance(root, k, H)
    state, (steps, ticks) = root.get_state(), root.get_counters()
    beam = planning.BeamPlanner(root, width=width, horizon=H, gamma=gamma, substeps=k)
    actions, _ = beam.plan_host()
    slots, host_actions, near = _host_beam(cfg, state, steps, ticks, n, width, H, k, beam.weights)
    print("near-ties skipped: %d of %d roots" % (int(near.sum()), n))
    ok = ~near
    assert ok.sum() >= n // 2
    assert np.array_equal(actions[ok], host_actions[ok])
    got = beam.last_beam_values()[ok]
    want = slots["value"].reshape(n, width)[ok]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.allclose(got, want, rtol=1e-11, atol=0.0, equal_nan=True)
    beam.close()
    root.close()


def test_planned_steps_replay_from_one_graph():
    import torch
    n, k, width, H = 64, 10, 3, 4
    cfg = default_config(4, GRAV_PM_J2)
    cfg.max_length = 1000
    side = torch.cuda.Stream()
    ic = sample_ic_batch(n, 4, seed=78)
    with torch.cuda.stream(side):
        g_root = BatchedPropagator(cfg, n, stream=side.cuda_stream)
        e_root = BatchedPropagator(cfg, n, stream=side.cuda_stream)
        for p in (g_root, e_root):
            p.reset(ic)
        g_plan = planning.BeamPlanner(g_root, width=width, horizon=H, substeps=k)
        e_plan = planning.BeamPlanner(e_root, width=width, horizon=H, substeps=k)
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
        assert np.array_equal(g_plan.last_beam_values(), e_plan.last_beam_values(), equal_nan=True)
        assert np.array_equal(g_root.get_state(), e_root.get_state())
        for a, b in zip(g_root.get_obs(), e_root.get_obs()):
            assert np.array_equal(a, b)
        assert np.array_equal(g_root.get_counters()[1], np.full(n, 3 * k))
        del graph
        for x in (g_plan, e_plan, g_root, e_root):
            x.close()
