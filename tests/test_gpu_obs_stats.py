"""GPU: running observation statistics on the device and the input normalisation out of them (bsk_obs_stats_*,
bsk_*_set_obs_stats, bsk_es_apply_obs_norm; kernels in csrc/bsk_obsstats.hip; contract in include/bskgpu.h).

Every check is an EQUALITY of bits against the numpy restatement (policy.obs_stats_accumulate_ref / obs_stats_totals_ref /
obs_norm_ref, which tests/test_obs_stats_host.py holds to exact rational arithmetic) or against code that already ships - no
tolerance anywhere.  Shapes: n = 64 is one wave; n = 100 in rows 128 apart has 28 tail lanes in its second wave (in an object of
capacity 200: two partial rows nobody writes); n = 8320 is 130 waves, so the join's lanes 0 and 1 add three partial rows and the
others two.  Magnitudes are spread over 1e-6 .. 1e3, so that a product contracted into the sum behind it would show.
"""
import ctypes

import numpy as np
import pytest

from _device_bits import download as _download, same as _same
from _policy_bounds import seeded_policy
from basilisk_env_amd import _hip, _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch

pytestmark = pytest.mark.gpu


def _upload(buf, arr):
    arr = np.ascontiguousarray(arr)
    assert arr.nbytes <= buf.nbytes
    _hip.check(_hip.runtime().hipMemcpy(ctypes.c_void_p(buf.ptr), ctypes.c_void_p(arr.ctypes.data), arr.nbytes, _hip.hipMemcpyHostToDevice), "hipMemcpy")


def _block(rng, n):
    """(5, n) float64 of either sign, magnitudes spread over 1e-6 .. 1e3, a few signed zeros among them"""
    x = np.where(rng.random((5, n)) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6.0, 3.0, (5, n))
    x[rng.integers(0, 5, 3), rng.integers(0, n, 3)] = -0.0
    return x


def _totals(stats):
    """(tot float64 (10,), count) read from the object's device words; the caller has synchronised"""
    t, c = stats.totals_ptr()
    return _download(t, np.float64, 10), int(_download(c, np.uint64, 1)[0])


def _holds(stats, state):
    """the device object holds exactly `state` = (part, cnt), with the totals, count, mean and var that follow from it"""
    part, cnt = stats.state                                  # (synchronises the device)
    assert part.shape == state[0].shape and _same(part, state[0]) and _same(cnt, state[1])
    tot, count = P.obs_stats_totals_ref(state)
    got_tot, got_count = _totals(stats)
    assert _same(got_tot, tot) and got_count == count == stats.count
    if count:
        mean, var = P.obs_moments_ref(tot, count)
        assert _same(stats.mean, mean) and _same(stats.var, var)
    else:
        assert _same(stats.mean, np.zeros(5)) and _same(stats.var, np.zeros(5))
    return tot, count


@pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])
@pytest.mark.parametrize("n,stride,n_cap", [(64, 64, 64), (100, 128, 200), (8320, 8320, 8320)])
def test_accumulate_equals_the_definition_call_after_call(n, stride, n_cap, masked):
    rng = np.random.default_rng(1000 * n + masked)
    stats = P.ObsStats(n_cap)
    d_obs, d_alive = _hip.DeviceBuffer(5 * stride * 8, 0), _hip.DeviceBuffer(n, 0)
    state = P.obs_stats_zero_state(n_cap)
    assert stats.waves == state[0].shape[0] == (n_cap + 63) // 64
    _holds(stats, state)                                     # all zero after creation
    waves = (n + 63) // 64
    for call in range(3):
        obs = _block(rng, n)
        rows = np.full((5, stride), np.nan)                  # (what lies between the rows is never read into a sum)
        rows[:, :n] = obs
        _upload(d_obs, rows)
        alive = None
        if masked:
            alive = (rng.random(n) < 0.7).astype(np.uint8) * np.uint8(1 + 127 * (call % 2))      # (any non-zero byte is alive)
            alive[64 * (call % waves):][:64] = 0             # one wholly dead wave
            _upload(d_alive, alive)
        c0 = BatchedPropagator.debug_counters()
        stats.accumulate(d_obs.ptr, n, stride, d_alive.ptr if masked else None)
        assert BatchedPropagator.debug_counters() == c0      # enqueue only
        state = P.obs_stats_accumulate_ref(state, obs, alive)
        tot, count = _holds(stats, state)
        assert np.isfinite(tot).all() and (count > 0 or (masked and n == 64))
    if masked and n == 64:
        assert count == 0 and not state[0].any()             # its only wave was dead in every call: nothing was ever stored
    else:
        assert count > 0 and (tot[5:] > 0).all()
    # the checkpoint: the state into a second object - totals formed again - and both carried one call further
    twin = P.ObsStats(n_cap)
    twin.set_state(*state)
    _holds(twin, state)
    obs = _block(rng, n)
    rows = np.full((5, stride), np.nan)
    rows[:, :n] = obs
    _upload(d_obs, rows)
    for s in (stats, twin):
        s.accumulate(d_obs.ptr, n, stride)
    state = P.obs_stats_accumulate_ref(state, obs, None)
    _holds(stats, state)
    _holds(twin, state)
    # an array in place of the raw pointer, and reset
    import torch
    t = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    twin.reset()
    twin.accumulate(t[:, :n])
    _holds(twin, P.obs_stats_accumulate_ref(P.obs_stats_zero_state(n_cap), obs, None))
    for x in (stats, twin):
        x.close()
    d_obs.free()
    d_alive.free()


def _propagator(n, ic, max_length, stream=None, stagger=0):
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    cfg.max_length = max_length
    p = BatchedPropagator(cfg, n, stream=stream)
    p.set_ic_pool(sample_ic_batch(41, 4, seed=15))
    p.reset(ic)
    p.step(np.zeros(n, np.int32), 1)
    if stagger:              # the envs are `env mod stagger` steps into their episodes: they end by length at different steps
        p.sync()
        _, ticks = p.get_counters()
        p.set_counters((np.arange(n) % stagger).astype(np.int32), ticks)
    return p


def _envs(p):
    p.sync()
    out = {"state": p.get_state()}
    out["steps"], out["ticks"] = p.get_counters()
    out["obs"], out["rew"], _, out["why"] = p.get_obs()
    out["term_obs"], out["episodes"] = p.get_terminal_obs()
    return out


HIST = (("obs", 40, np.float64), ("reward", 8, np.float64), ("reason", 1, np.uint8), ("action", 4, np.int32), ("logp", 4, np.float32))


def _population_rollout(pop, prop, T, n, n_members, fitness=True):
    import torch
    bufs = {key: torch.zeros(T * n * size, dtype=torch.uint8, device="cuda") for key, size, _ in HIST}
    outs = {"env_value": torch.full((n,), -7.0, dtype=torch.float64, device="cuda"),
            "env_len": torch.full((n,), -7, dtype=torch.int32, device="cuda"),
            "fitness": torch.full((n_members,), -7.0, dtype=torch.float64, device="cuda"),
            "mean_len": torch.full((n_members,), -7.0, dtype=torch.float64, device="cuda")}
    torch.cuda.synchronize()
    kw = {"d_" + key: val.data_ptr() for key, val in outs.items()} if fitness else {}
    c0 = BatchedPropagator.debug_counters()
    pop.rollout_device(prop, T, 1, "greedy", 0.97, *(bufs[key].data_ptr() for key, _, _ in HIST), None, **kw)
    assert BatchedPropagator.debug_counters() == c0          # enqueue only, with or without statistics attached
    prop.sync()
    got = {key: bufs[key].cpu().numpy().view(dt).reshape((T, 5, n) if key == "obs" else (T, n)) for key, _, dt in HIST}
    got.update({key: val.cpu().numpy() for key, val in outs.items()})
    return got


def test_a_population_rollout_counts_the_episode_that_counts_towards_fitness():
    n_members, T = 2, 6
    n = 8320                                                 # 65 waves per member, 130 partial rows
    spec, _ = seeded_policy((16,), "relu", None, seed=3)
    params = np.stack([seeded_policy((16,), "relu", None, seed=3 + 17 * m)[1] for m in range(n_members)])
    ic = sample_ic_batch(n, 4, seed=14)
    pop = P.PolicyPopulation(spec, params)
    stats = P.ObsStats(n)
    runs = {}
    for attached in (True, False):
        prop = _propagator(n, ic, max_length=7, stagger=8)
        obs0 = prop.get_obs()[0]
        pop.set_obs_stats(stats if attached else None)
        got = _population_rollout(pop, prop, T, n, n_members)
        runs[attached] = (got, _envs(prop), obs0)
        prop.close()
    got, _, obs0 = runs[True]
    # the case: some envs ended inside the rollout - and went on, restarted, with observations that do not count - others did not
    assert (got["env_len"] < T).any() and (got["env_len"] == T).any() and got["env_len"].min() >= 1
    assert len(set(got["env_len"].tolist())) >= 3
    state = P.obs_stats_zero_state(n)
    for t in range(T):
        alive = None if t == 0 else (got["reason"][:t] == 0).all(axis=0).astype(np.uint8)
        state = P.obs_stats_accumulate_ref(state, obs0 if t == 0 else got["obs"][t - 1], alive)
    _, count = _holds(stats, state)
    assert count == int(got["env_len"].sum()) and n < count < T * n
    # nothing but the statistics differs from the same rollout with nothing attached
    for key in got:
        assert _same(got[key], runs[False][0][key]), key
    for key in runs[True][1]:
        assert _same(runs[True][1][key], runs[False][1][key]), key
    assert _same(obs0, runs[False][2])
    _holds(stats, state)                                     # (the detached rollout left the object alone)
    # a rollout that forms no fitness counts every env at every step
    stats.reset()
    pop.set_obs_stats(stats)
    prop = _propagator(n, ic, max_length=7, stagger=8)
    got = _population_rollout(pop, prop, T, n, n_members, fitness=False)
    state = P.obs_stats_zero_state(n)
    for t in range(T):
        state = P.obs_stats_accumulate_ref(state, obs0 if t == 0 else got["obs"][t - 1], None)
    assert _holds(stats, state)[1] == T * n
    pop.set_obs_stats(None)
    for x in (prop, pop, stats):
        x.close()


def test_a_policy_rollout_counts_every_env_at_every_step():
    n, T = 200, 5                                            # (three full waves and a tail of eight lanes)
    spec, params = seeded_policy((16,), "relu", None, seed=8)
    ic = sample_ic_batch(n, 4, seed=23)
    pol = P.DevicePolicy(spec, params)
    stats = P.ObsStats(256)
    runs = {}
    for attached in (True, False):
        prop = _propagator(n, ic, max_length=3)
        obs0 = prop.get_obs()[0]
        pol.set_obs_stats(stats if attached else None)
        runs[attached] = (pol.rollout(prop, T, 1, "greedy"), _envs(prop))
        prop.close()
    got = runs[True][0]
    assert (got["reason"] != 0).any()                        # episodes ended and restarted inside the rollout: they count all the same
    state = P.obs_stats_zero_state(256)
    for t in range(T):
        state = P.obs_stats_accumulate_ref(state, obs0 if t == 0 else got["obs"][t - 1], None)
    assert _holds(stats, state)[1] == T * n
    for key in got:
        assert _same(got[key], runs[False][0][key]), key
    for key in runs[True][1]:
        assert _same(runs[True][1][key], runs[False][1][key]), key
    for x in (pol, stats):
        x.close()


def test_apply_obs_norm_writes_the_definition_into_theta():
    n, n_members = 1000, 4
    spec, theta0 = seeded_policy((16,), "relu", None, seed=9)
    es = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=0.1, lr=0.05, seed=5, frozen=10)
    pop = P.PolicyPopulation(spec, n_members=n_members)
    stats = P.ObsStats(n)
    want = theta0.astype(np.float64)
    # nothing counted yet: nothing is written
    es.apply_obs_norm(stats)
    assert _same(es.theta, want)
    rng = np.random.default_rng(12)
    obs = _block(rng, n) + np.array([0.0, 5.0, -300.0, 1e-3, 0.0])[:, None]
    obs[4] = 0.625                                           # a row that has not varied - and one that barely has
    obs[3] = 1e-8 * (rng.random(n) - 0.5)
    d_obs = _hip.DeviceBuffer(obs.nbytes, 0)
    _upload(d_obs, obs)
    stats.accumulate(d_obs.ptr, n)
    c0 = BatchedPropagator.debug_counters()
    es.apply_obs_norm(stats, std_min=1e-6)
    assert BatchedPropagator.debug_counters() == c0
    tot, count = P.obs_stats_totals_ref(P.obs_stats_accumulate_ref(P.obs_stats_zero_state(n), obs, None))
    scale, shift = P.obs_norm_ref(tot, count, 1e-6)
    want[:5], want[5:10] = scale, shift
    got = es.theta
    assert _same(got[:10], want[:10]) and _same(got[10:], theta0[10:].astype(np.float64))
    assert (scale[:3] > 0).all() and scale[3] == 0.0 and scale[4] == 0.0 and _same(shift[3:], np.zeros(2)) and (shift[:3] != 0).all()
    # a smaller std_min lets the fourth row through: the threshold is an argument, not a constant of the kernel
    es.apply_obs_norm(stats, std_min=1e-12)
    s2, h2 = P.obs_norm_ref(tot, count, 1e-12)
    assert s2[3] > 1e6 and _same(es.theta[:10], np.r_[s2, h2])
    es.apply_obs_norm(stats, std_min=1e-6)
    # the next ask carries the ten floats into every member
    es.ask(pop)
    members = np.stack([pop.member(m) for m in range(n_members)])
    assert _same(members[:, :10], np.broadcast_to(want[:10].astype(np.float32), (n_members, 10)))
    assert _same(members, P.es_ask_ref(want, 0.1, 10, n_members, 5, 0))
    for x in (es, pop, stats):
        x.close()
    d_obs.free()


def test_generations_with_statistics_replay_from_a_hip_graph():
    import torch
    n_members, E, T = 4, 64, 8
    n = n_members * E
    spec, theta0 = seeded_policy((16,), "tanh", None, seed=5)
    ic = sample_ic_batch(n, 4, seed=29)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        def make():
            prop = _propagator(n, ic, max_length=6, stream=side.cuda_stream)
            pop = P.PolicyPopulation(spec, n_members=n_members)
            es = P.DeviceEvolutionStrategy(spec, theta0, n_members, sigma=0.1, lr=0.05, seed=3, frozen=10)
            stats = P.ObsStats(n)
            es.run_generation(prop, pop, T, 1, "greedy", 0.99, obs_stats=stats)          # the warming call
            prop.sync()
            return prop, pop, es, stats

        def state(es, stats):
            theta = es.theta                                 # (synchronises the device)
            return (theta,) + stats.state + _totals(stats) + (es.generation,)

        prop, pop, es, stats = make()
        first = state(es, stats)
        assert first[-1] == 1 and first[4] > 0 and not _same(first[0][:10], theta0[:10].astype(np.float64))
        eager = []
        for g in range(3):
            c0 = BatchedPropagator.debug_counters()
            es.run_generation(prop, pop, T, 1, "greedy", 0.99, obs_stats=stats)
            assert BatchedPropagator.debug_counters() == c0  # no copy, no synchronisation
            eager.append(state(es, stats))
            assert getattr(pop, "_stats", None) is None      # the population is left as it was found
        assert eager[2][-1] == 4 and eager[0][4] < eager[1][4] < eager[2][4]
        assert not _same(eager[0][0], eager[1][0]) and not _same(eager[1][0][:10], eager[2][0][:10])
        for x in (prop, pop, es, stats):
            x.close()

        prop, pop, es, stats = make()
        warm = state(es, stats)
        assert all(_same(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(warm, first))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            es.run_generation(prop, pop, T, 1, "greedy", 0.99, obs_stats=stats)
        for g in range(3):
            c0 = BatchedPropagator.debug_counters()
            graph.replay()
            torch.cuda.synchronize()
            assert BatchedPropagator.debug_counters() == c0
            got = state(es, stats)
            for a, b in zip(got, eager[g]):
                assert _same(a, b) if isinstance(a, np.ndarray) else a == b, g
        for x in (prop, pop, es, stats):
            x.close()


def test_refusals_come_before_any_launch():
    lib = _lib.load()
    n = 128
    spec, theta0 = seeded_policy((16,), "relu", None, seed=21)
    nan, inf = float("nan"), float("inf")
    h = ctypes.c_void_p()
    for n_cap in (0, -5, (1 << 28) + 1):
        assert lib.bsk_obs_stats_create(n_cap, 0, ctypes.byref(h)) == -1 and not h.value
    assert lib.bsk_obs_stats_create(64, 0, None) == -1
    with pytest.raises(_lib.BskGpuUnavailable):
        P.ObsStats(64, device=_hip.device_count())

    stats = P.ObsStats(n)
    rng = np.random.default_rng(2)
    obs = _block(rng, n)
    d_obs = _hip.DeviceBuffer(obs.nbytes, 0)
    _upload(d_obs, obs)
    stats.accumulate(d_obs.ptr, n)
    kept = P.obs_stats_accumulate_ref(P.obs_stats_zero_state(n), obs, None)
    _holds(stats, kept)
    es = P.DeviceEvolutionStrategy(spec, theta0, 2, frozen=10)
    thawed = P.DeviceEvolutionStrategy(spec, theta0, 2, frozen=9)
    pop = P.PolicyPopulation(spec, n_members=2)
    pol = P.DevicePolicy(spec, theta0)
    prop = _propagator(4 * n, sample_ic_batch(4 * n, 4, seed=3), max_length=5)          # more envs than the object has room for
    before = _envs(prop)
    s, e, o = stats._handle(), es._handle(), ctypes.c_void_p(d_obs.ptr)
    c0 = BatchedPropagator.debug_counters()
    for args in ((None, o, n, n, None), (s, None, n, n, None), (s, o, n, 0, None), (s, o, n, -3, None), (s, o, n + 64, n + 1, None),
                 (s, o, n - 1, n, None), (s, o, 5, 64, None)):
        assert lib.bsk_obs_stats_accumulate(*args, None) == -1, args
        assert lib.bsk_last_error()
    for args in ((None, s, 1e-6), (e, None, 1e-6), (thawed._handle(), s, 1e-6), (e, s, 0.0), (e, s, -1e-6), (e, s, nan), (e, s, inf)):
        assert lib.bsk_es_apply_obs_norm(*args, None) == -1, args
        assert lib.bsk_last_error()
    assert lib.bsk_population_set_obs_stats(None, s) == -1 and lib.bsk_policy_set_obs_stats(None, s) == -1
    assert lib.bsk_obs_stats_reset(None, None) == -1 and lib.bsk_obs_stats_get(None, None, None, None) == -1
    assert lib.bsk_obs_stats_get_state(None, None, None) == -1 and lib.bsk_obs_stats_set_state(None, None, None) == -1
    assert lib.bsk_obs_stats_set_state(s, kept[0].ctypes.data, None) == -1 and lib.bsk_obs_stats_set_state(s, None, kept[1].ctypes.data) == -1
    assert lib.bsk_obs_stats_totals_device(s, None, None) == -1 and lib.bsk_obs_stats_totals_device(None, ctypes.byref(h), ctypes.byref(h)) == -1
    # attached to something whose handle is larger than the object: the rollouts refuse, with nothing enqueued
    pop.set_obs_stats(stats)
    pol.set_obs_stats(stats)
    with pytest.raises(_lib.BskError, match="capacity"):
        pop.rollout_device(prop, 3, 1)
    with pytest.raises(_lib.BskError, match="capacity"):
        pol.rollout_device(prop, 3, 1)
    assert BatchedPropagator.debug_counters() == c0
    after = _envs(prop)
    for key in before:
        assert _same(before[key], after[key]), key
    _holds(stats, kept)                                      # nothing was launched: the state is what it was
    assert _same(es.theta, theta0.astype(np.float64)) and _same(thawed.theta, theta0.astype(np.float64))
    if _hip.device_count() > 1:
        far = P.ObsStats(4 * n, device=1)
        assert lib.bsk_es_apply_obs_norm(e, far._handle(), 1e-6, None) == -1 and b"different devices" in lib.bsk_last_error()
        pop.set_obs_stats(far)
        with pytest.raises(_lib.BskError, match="different devices"):
            pop.rollout_device(prop, 3, 1)
        pop.set_obs_stats(None)
        far.close()
    # ... and detached, or with legal arguments, the same calls do run
    pop.set_obs_stats(None)
    pol.set_obs_stats(None)
    pop.rollout_device(prop, 3, 1)
    es.apply_obs_norm(stats)
    prop.sync()
    scale, shift = P.obs_norm_ref(*P.obs_stats_totals_ref(kept), 1e-6)
    assert _same(es.theta[:10], np.r_[scale, shift])
    _holds(stats, kept)
    for x in (prop, pop, pol, es, thawed, stats):
        x.close()
    d_obs.free()
    with pytest.raises(RuntimeError, match="observation statistics is closed"):
        stats.accumulate(0, 1)
