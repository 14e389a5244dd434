"""GPU: the fused MLP policy (bsk_policy_*, csrc/bsk_policy.hip; contract in include/bskgpu.h) against its numpy restatement
(basilisk_env_amd/policy.py).

`relu` and linear networks are held bit for bit - logits, value, greedy actions - because the definition fixes every layer output as one
k-ordered chain of f32 fused multiply-adds.  What goes through tanhf / expf / logf is held within bounds DERIVED in
tests/_policy_bounds.py (no tolerance here was picked because the kernel met it), and where a decision could go either way inside
such a bound (two logits closer than twice the bound, u within delta of a CDF boundary) either outcome is accepted - for at most
0.1 % of the spacecraft; the shares are printed.  Closed loops (bsk_policy_rollout, LeoPowerAttVecEnv.step_policy) are compared with
a host-driven loop that reads the observation back, chooses with act_ref and steps with those actions.
"""

import numpy as np
import pytest

from _device_bits import download as _download
from _policy_bounds import centred, mlp_bound, observation_like, reset_observations, seeded_policy, softmax_bound
from basilisk_env_amd import _hip, _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET, FLAG_DESAT, FLAG_DRAG, FLAG_POWER, FLAG_SUN_THIRD_BODY, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch

pytestmark = pytest.mark.gpu

FULL = FLAG_POWER | FLAG_SUN_THIRD_BODY | FLAG_DRAG | FLAG_DESAT
SIZES = (1, 63, 64, 65, 777, 65536 + 77)
CAP = 1e-3            # at most 0.1 % of the spacecraft may fall inside a bound's either-way zone


def _host(view, sync):
    """a device view of the policy (or a propagator) -> numpy, after `sync` (an object with .sync()) has drained its stream"""
    sync.sync()
    a = view.__cuda_array_interface__
    dt = np.dtype(a["typestr"])
    assert a["strides"] is None
    return _download(a["data"][0], dt, int(np.prod(a["shape"]))).reshape(a["shape"])


def _device_obs(obs, pad):
    """(5, n) host observations -> a torch tensor view (5, n) of a (5, n + pad) device block: rows n + pad apart"""
    import torch
    n = obs.shape[1]
    block = torch.full((5, n + pad), float("nan"), dtype=torch.float64, device="cuda")
    block[:, :n] = torch.from_numpy(np.ascontiguousarray(obs)).cuda()
    torch.cuda.synchronize()
    return block[:, :n]


def _run(pol, source, mode="greedy", want=("logp", "value", "logits"), **kw):
    res = pol.act(source, mode, want, **kw)
    sync = getattr(source, "propagator", source) if hasattr(source, "sync") else pol
    return {k: _host(v, sync) for k, v in res.items()}


@pytest.mark.parametrize("hidden", [(), (16,), (64, 64), (128, 128, 128), (48, 112)], ids=str)
@pytest.mark.parametrize("value", [False, True], ids=["action-only", "with-value"])
def test_relu_and_linear_networks_bit_for_bit(hidden, value):
    spec, params = seeded_policy(hidden, "relu", hidden if value else None, seed=len(hidden))
    pol = P.DevicePolicy(spec, params)
    want = ("logp", "value", "logits") if value else ("logp", "logits")
    for n in SIZES:
        obs = observation_like(n, seed=n)
        got = _run(pol, _device_obs(obs, 0 if n == 64 else 131), "greedy", want)
        l, v = P.mlp_ref(spec, params, obs)
        a, _ = P.act_ref(l, "greedy")
        assert np.array_equal(got["logits"], l), (hidden, n)
        assert np.array_equal(got["action"], a), (hidden, n)
        if value:
            assert np.array_equal(got["value"], v), (hidden, n)
        # the log-probability of the chosen action, within its derived bound of fp64 on the same f32 logits
        _, _, logp, _, e_logp = softmax_bound(l)
        j = np.arange(n)
        assert np.all(np.abs(got["logp"].astype(np.float64) - logp[a, j]) <= e_logp[a, j]), (hidden, n)
    pol.close()


def test_exact_ties_go_to_the_lowest_index_and_tail_lanes_store_nothing():
    import torch
    spec, params = seeded_policy((64, 64), "relu", None, seed=3)
    sc, sh, layers, _ = P.unpack_params(spec, params)
    W, b = layers[-1][0].copy(), layers[-1][1].copy()
    n = 777
    obs = observation_like(n, seed=5)
    for dup, never in (((0, 1), 1), ((1, 2), 2), ((0, 2), 2)):
        W2, b2 = W.copy(), b.copy()
        W2[dup[1]], b2[dup[1]] = W2[dup[0]], b2[dup[0]]          # two output rows equal: their logits tie exactly, everywhere
        p2 = P.pack_params(spec, layers[:-1] + [(W2, b2)], None, sc, sh)
        pol = P.DevicePolicy(spec, p2)
        got = _run(pol, _device_obs(obs, 50), "greedy", ("logits",))
        assert np.array_equal(got["logits"][dup[0]], got["logits"][dup[1]])
        l, _ = P.mlp_ref(spec, p2, obs)
        a, _ = P.act_ref(l, "greedy")
        assert np.array_equal(got["action"], a) and not np.any(got["action"] == never) and np.any(got["action"] == dup[0])
        pol.close()
    # raw entry point with outputs the test owns: nothing beyond n is written (actions, logp, and every logits row)
    pol = P.DevicePolicy(spec, params)
    lib = _lib.load()
    d_obs = _device_obs(obs, 23)
    act = torch.full((n + 64,), -7, dtype=torch.int32, device="cuda")
    logp = torch.full((n + 64,), -7.0, dtype=torch.float32, device="cuda")
    logits = torch.full((3, n + 64), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(lib.bsk_policy_act(pol._handle(), d_obs.data_ptr(), d_obs.stride(0), n, 0, 0, act.data_ptr(), logp.data_ptr(), None,
                                  logits.data_ptr(), n + 64, None))
    torch.cuda.synchronize()
    l, _ = P.mlp_ref(spec, params, obs)
    assert np.array_equal(logits[:, :n].cpu().numpy(), l) and bool((logits[:, n:] == -7).all())
    assert bool((act[n:] == -7).all()) and bool((logp[n:] == -7).all()) and int(act[:n].min()) >= 0 and int(act[:n].max()) <= 2
    # non-finite observations: outside the numerical contract, but the action stays in {0, 1, 2}
    bad = obs.copy()
    bad[:, ::3] = np.nan
    bad[1, 1::3] = np.inf
    for mode in ("greedy", "sample"):
        a = _run(pol, _device_obs(bad, 0), mode, ())["action"]
        assert a.min() >= 0 and a.max() <= 2
    pol.close()


def _stepped_propagator(n, steps=3, flags=0, k=2, max_length=None, seed=4):
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= flags
    if max_length:
        cfg.max_length = max_length
    p = BatchedPropagator(cfg, n)
    if flags & FLAG_AUTO_RESET:
        p.set_ic_pool(sample_ic_batch(41, 4, seed=seed + 1))
    p.reset(sample_ic_batch(n, 4, seed=seed))
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        p.step(rng.integers(0, 3, n).astype(np.int32), k)
    return p


def _loop_policy(hidden, value_hidden, seed):
    """a seeded relu policy whose three actions all occur on the env's observations (output biases centred on reset observations)"""
    spec, params = seeded_policy(hidden, "relu", value_hidden, seed=seed)
    return spec, centred(spec, params, reset_observations(sample_ic_batch(2000, 4, seed=0), default_config(4, GRAV_PM_J2)))


@pytest.mark.parametrize("n", [1, 65, 777, 5000])
def test_real_observation_buffers_bit_for_bit(n):
    prop = _stepped_propagator(n, flags=FLAG_POWER)
    spec, params = _loop_policy((64, 64), (64, 64), 8)
    pol = P.DevicePolicy(spec, params)
    got = _run(pol, prop)
    obs = prop.get_obs()[0]
    l, v = P.mlp_ref(spec, params, obs)
    a, _ = P.act_ref(l, "greedy")
    assert np.array_equal(got["logits"], l) and np.array_equal(got["value"], v) and np.array_equal(got["action"], a)
    assert len(set(a.tolist())) > 1 or n == 1
    # the action view's pointer is what step_device reads, in place: the same step as the host's actions give
    twin = _stepped_propagator(n, flags=FLAG_POWER)
    res = pol.act(prop, "greedy", ())
    prop.step_device(res["action"].__cuda_array_interface__["data"][0], 2)
    twin.step(a, 2)
    assert np.array_equal(prop.get_state(), twin.get_state()) and np.array_equal(prop.get_obs()[0], twin.get_obs()[0])
    for p in (prop, twin, pol):
        p.close()


@pytest.mark.parametrize("hidden,value", [((64, 64), (64, 64)), ((48, 112), None), ((128, 128, 128), (16,)), ((16,), (128, 128))], ids=str)
def test_tanh_networks_within_the_derived_bound(hidden, value):
    spec, params = seeded_policy(hidden, "tanh", value, seed=11)
    pol = P.DevicePolicy(spec, params)
    want = ("logp", "value", "logits") if value else ("logp", "logits")
    for n in (1, 63, 64, 65, 777, 1 << 17):
        obs = observation_like(n, seed=n + 1)
        got = _run(pol, _device_obs(obs, 77), "greedy", want)
        l64, e_l, v64, e_v = mlp_bound(spec, params, obs)
        err = np.abs(got["logits"].astype(np.float64) - l64)
        print("tanh %s n=%d: logits max error %.3g, max error / bound %.3f" % (hidden, n, err.max(), (err / e_l).max()))
        assert np.all(err <= e_l)
        if value:
            assert np.all(np.abs(got["value"].astype(np.float64) - v64) <= e_v)
        # greedy: numpy's choice wherever the fp64 top-two margin exceeds twice the bound, one of the near-tied candidates elsewhere
        order = np.argsort(-l64, axis=0, kind="stable")
        j = np.arange(n)
        top, second = l64[order[0], j], l64[order[1], j]
        bound = e_l.max(axis=0)
        clear = (top - second) > 2 * bound
        assert np.array_equal(got["action"][clear], order[0][clear])
        near = l64 >= top - 2 * bound                       # the candidates within the either-way zone of the leader
        assert np.all(near[got["action"], j])
        share = 1.0 - clear.mean()
        print("tanh %s n=%d: %.4f %% of spacecraft under the margin (cap 0.1 %%)" % (hidden, n, 100 * share))
        if n >= 1000:
            assert share <= CAP
    pol.close()


def test_sampled_actions_logp_and_the_draw_counter():
    spec, params = seeded_policy((64, 64), "relu", None, seed=21)
    pol = P.DevicePolicy(spec, params)
    n = 1 << 17
    obs = observation_like(n, seed=9)
    d_obs = _device_obs(obs, 0)
    l, _ = P.mlp_ref(spec, params, obs)
    c0, c1, logp64, delta, e_logp = softmax_bound(l)
    j = np.arange(n)
    assert pol.get_rng() == (0, 0)
    pol.set_rng(seed=(0xABCDEF << 20) + 5, draw=(1 << 35) + 7)
    seed, draw = pol.get_rng()
    assert (seed, draw) == ((0xABCDEF << 20) + 5, (1 << 35) + 7)
    runs = []
    for call in range(3):
        base = 1000 * call
        got = _run(pol, d_obs, "sample", ("logp", "logits"), env_base=base)
        assert np.array_equal(got["logits"], l)
        u = P.sample_uniform(n, seed, draw + call, base).astype(np.float64)
        clear = (np.abs(u - c0) > delta) & (np.abs(u - c1) > delta)
        a64 = np.where(u < c0, 0, np.where(u < c1, 1, 2))
        a_ref, _ = P.act_ref(l, "sample", seed, draw + call, base)
        assert np.array_equal(got["action"][clear], a64[clear]) and np.array_equal(a_ref[clear], a64[clear])
        assert np.all(np.abs(got["action"] - a64) <= 1) and got["action"].min() >= 0 and got["action"].max() <= 2
        share = 1.0 - clear.mean()
        print("sample call %d: %.4f %% of spacecraft within delta of a CDF boundary (cap 0.1 %%), max delta %.3g" % (call, 100 * share, delta.max()))
        assert share <= CAP
        assert np.all(np.abs(got["logp"].astype(np.float64) - logp64[got["action"], j]) <= e_logp[got["action"], j])
        assert pol.get_rng() == (seed, draw + call + 1)       # +1 per sample-mode call, on the device
        runs.append(got["action"])
    assert 0.2 < np.mean(runs[0] != runs[1]) < 0.9            # new numbers per call
    _run(pol, d_obs, "greedy", ())
    assert pol.get_rng() == (seed, draw + 3)                  # +0 per greedy call
    pol.set_rng(seed, draw)
    again = _run(pol, d_obs, "sample", (), env_base=0)["action"]
    assert np.array_equal(again, runs[0])                     # set_rng replays
    # shard independence: env j of a call with env_base = b is env 0 of a call with env_base = b + j (64-bit bases included)
    for b in (0, 12345, (1 << 32) - 2, (1 << 41) + 3):
        pol.set_rng(seed, draw)
        whole = _run(pol, d_obs[:, :256], "sample", (), env_base=b)["action"]
        for jj in (1, 63, 64, 200):
            pol.set_rng(seed, draw)
            part = _run(pol, d_obs[:, jj:jj + 3], "sample", (), env_base=b + jj)["action"]
            assert np.array_equal(part, whole[jj:jj + 3]), (b, jj)
    pol.close()


def test_set_params_replaces_the_network():
    spec, p1 = seeded_policy((16,), "relu", (16,), seed=1)
    _, p2 = seeded_policy((16,), "relu", (16,), seed=2)
    pol = P.DevicePolicy(spec, p1)
    obs = observation_like(300, seed=1)
    d_obs = _device_obs(obs, 4)
    for params in (p1, p2, p1):
        pol.set_params(params)
        got = _run(pol, d_obs)
        l, v = P.mlp_ref(spec, params, obs)
        assert np.array_equal(got["logits"], l) and np.array_equal(got["value"], v)
    with pytest.raises(ValueError):
        pol.set_params(p1[:-1])
    pol.close()


def test_from_torch_on_the_device():
    import torch
    nn = torch.nn
    torch.manual_seed(2)
    net = nn.Sequential(nn.Linear(5, 64), nn.Tanh(), nn.Linear(64, 64), nn.Tanh(), nn.Linear(64, 3))
    val = nn.Sequential(nn.Linear(5, 32), nn.ReLU(), nn.Linear(32, 1))
    pol = P.DevicePolicy.from_torch(net, val)
    assert pol.spec == P.check_spec((64, 64), "tanh", (32,), "relu")
    obs = observation_like(2000, seed=3)
    got = _run(pol, _device_obs(obs, 0))
    hidden, act, layers = P.torch_layers(net)
    params = P.pack_params(pol.spec, layers, P.torch_layers(val)[2])
    l64, e_l, v64, e_v = mlp_bound(pol.spec, params, obs)
    assert np.all(np.abs(got["logits"] - l64) <= e_l) and np.all(np.abs(got["value"] - v64) <= e_v)
    with torch.no_grad():
        x = torch.from_numpy(obs.T.astype(np.float32))
        tl = net(x).numpy().T.astype(np.float64)
    assert np.all(np.abs(got["logits"] - tl) <= 2 * e_l)       # (torch's own f32 forward obeys the same bound)
    pol.close()


def _envs(p):
    p.sync()
    out = {"state": p.get_state()}
    out["steps"], out["ticks"] = p.get_counters()
    out["obs"], out["rew"], _, out["why"] = p.get_obs()
    v = p.device_views()
    out["done_mask"] = _download(v["done_mask"].__cuda_array_interface__["data"][0], np.uint64, (p.n_envs + 63) // 64)
    if "terminal_obs" in v:
        out["term_obs"], out["episodes"] = p.get_terminal_obs()
    return out


def _host_loop(prop, spec, params, T, k, mode="greedy", seed=0, draw=0, env_base=0):
    """the loop closed on the host: read the observation back, choose with act_ref, step with those actions"""
    hist = {"obs": [], "reward": [], "reason": [], "action": [], "logits": [], "value": []}
    for t in range(T):
        obs = prop.get_obs()[0]
        l, v = P.mlp_ref(spec, params, obs)
        a, _ = P.act_ref(l, mode, seed, draw + t, env_base)
        prop.step(a, k)
        o, r, _, why = prop.get_obs()
        for key, val in (("obs", o), ("reward", r), ("reason", why), ("action", a), ("logits", l), ("value", v)):
            hist[key].append(np.array(val))
    return {key: np.stack(val) for key, val in hist.items() if val[0].ndim}


def test_rollout_equals_a_host_driven_loop_with_auto_reset():
    n, T, k = 300, 26, 1
    spec, params = _loop_policy((64, 64), (16,), 31)
    pol = P.DevicePolicy(spec, params)
    a = _stepped_propagator(n, steps=0, flags=FLAG_AUTO_RESET, max_length=7, seed=14)
    b = _stepped_propagator(n, steps=0, flags=FLAG_AUTO_RESET, max_length=7, seed=14)
    c = _stepped_propagator(n, steps=0, flags=FLAG_AUTO_RESET, max_length=7, seed=14)
    for p in (a, b, c):
        p.step(np.zeros(n, np.int32), k)           # (observation buffers hold a step's output, not a reset's)
    c0 = BatchedPropagator.debug_counters()
    bufs = {key: _hip.DeviceBuffer(T * n * size, 0) for key, size in (("obs", 40), ("reward", 8), ("reason", 1), ("action", 4), ("logp", 4), ("value", 4))}
    pol.rollout_device(a, T, k, "greedy", *(bufs[key].ptr for key in ("obs", "reward", "reason", "action", "logp", "value")))
    pol.rollout_device(a, 1, k, "greedy")          # (and once into the policy's scratch row: allocates it, then enqueue-only too)
    c1 = BatchedPropagator.debug_counters()
    pol.rollout_device(a, 1, k, "greedy")
    assert BatchedPropagator.debug_counters() == c1 and c1 == c0      # no copy, no synchronisation, in any of them
    a.sync()
    got = {key: _download(bufs[key].ptr, dt, T * n * m).reshape((T, 5, n) if m == 5 else (T, n))
           for key, dt, m in (("obs", np.float64, 5), ("reward", np.float64, 1), ("reason", np.uint8, 1), ("action", np.int32, 1),
                              ("logp", np.float32, 1), ("value", np.float32, 1))}
    want = _host_loop(b, spec, params, T + 2, k)
    for key in ("obs", "reward", "reason", "action", "value"):
        assert np.array_equal(got[key], want[key][:T]), key
    assert (got["reason"] != 0).sum() >= 3 * n and len(set(got["action"].ravel().tolist())) > 1      # episodes ended, and restarted
    ea, eb = _envs(a), _envs(b)
    assert int(ea["episodes"].min()) >= 3
    for key in ea:
        assert np.array_equal(ea[key], eb[key]), key
    # log-probabilities belong to the observation the action was chosen from
    for t in (0, T - 1):
        _, _, logp64, _, e_logp = softmax_bound(want["logits"][t])
        j = np.arange(n)
        assert np.all(np.abs(got["logp"][t] - logp64[want["action"][t], j]) <= e_logp[want["action"][t], j])
    # the convenience form returns the same rows
    host = pol.rollout(c, T, k, "greedy")
    for key in ("obs", "reward", "reason", "action", "value", "logp"):
        assert np.array_equal(host[key], got[key]), key
    for p in (a, b, c, pol):
        p.close()
    for buf in bufs.values():
        buf.free()


def test_rollout_full_scenario_at_the_reference_substeps():
    n, T, k = 96, 3, 1800
    spec, params = _loop_policy((16,), None, 41)
    pol = P.DevicePolicy(spec, params)
    a, b = (_stepped_propagator(n, steps=1, flags=FULL, k=k, seed=17) for _ in range(2))
    host = pol.rollout(a, T, k, "greedy")
    want = _host_loop(b, spec, params, T, k)
    for key in ("obs", "reward", "reason", "action"):
        assert np.array_equal(host[key], want[key]), key
    ea, eb = _envs(a), _envs(b)
    for key in ea:
        assert np.array_equal(ea[key], eb[key]), key
    assert "value" not in host and len(set(host["action"].ravel().tolist())) > 1
    for p in (a, b, pol):
        p.close()


def test_sampled_rollout_advances_the_draw_counter_and_uses_the_handles_env_base():
    n, T, k = 200, 5, 1
    spec, params = _loop_policy((16,), None, 51)
    pol = P.DevicePolicy(spec, params)
    a, b = (_stepped_propagator(n, steps=1, seed=19) for _ in range(2))
    a.set_env_base(5000)
    pol.set_rng(77, 10)
    host = pol.rollout(a, T, k, "sample")
    assert pol.get_rng() == (77, 10 + T)
    # host loop with the kernel's own logits replaced by numpy's (equal bit for bit); decisions compared away from the boundaries
    for t in range(T):
        obs = b.get_obs()[0]
        l, _ = P.mlp_ref(spec, params, obs)
        c0, c1, _, delta, _ = softmax_bound(l)
        u = P.sample_uniform(n, 77, 10 + t, 5000).astype(np.float64)
        clear = (np.abs(u - c0) > delta) & (np.abs(u - c1) > delta)
        a64 = np.where(u < c0, 0, np.where(u < c1, 1, 2))
        assert np.array_equal(host["action"][t][clear], a64[clear]) and clear.mean() > 0.99
        b.step(host["action"][t], k)               # (follow the device's choice where it was free to differ)
        assert np.array_equal(b.get_obs()[0], host["obs"][t])
    for p in (a, b, pol):
        p.close()


def test_act_and_rollout_replay_from_a_hip_graph():
    import torch
    n, k, inner, reps = 1000, 1, 4, 3
    spec, params = _loop_policy((64, 64), (64, 64), 61)
    side = torch.cuda.Stream()
    for mode in ("greedy", "sample"):
        with torch.cuda.stream(side):
            def make():
                cfg = default_config(4, GRAV_PM_J2)
                cfg.flags |= FLAG_AUTO_RESET
                cfg.max_length = 5
                p = BatchedPropagator(cfg, n, stream=side.cuda_stream)
                p.set_ic_pool(sample_ic_batch(41, 4, seed=3))
                p.reset(sample_ic_batch(n, 4, seed=2))
                pol = P.DevicePolicy(spec, params)
                pol.set_rng(9, 0)
                return p, pol

            def one(p, pol):
                res = pol.act(p, mode, ("logp", "value"))
                p.step_device(res["action"].__cuda_array_interface__["data"][0], k)
                pol.rollout_device(p, 2, k, mode)

            p, pol = make()
            for _ in range(inner * (reps + 1)):
                one(p, pol)
            want = _envs(p)
            want_rng = pol.get_rng()
            p.close()
            pol.close()

            p, pol = make()
            for _ in range(inner):                 # warm-up: the policy's buffers and scratch row are allocated outside the capture
                one(p, pol)
            p.sync()
            c0 = BatchedPropagator.debug_counters()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                for _ in range(inner):
                    one(p, pol)
            for _ in range(reps):
                graph.replay()
            torch.cuda.synchronize()
            assert BatchedPropagator.debug_counters() == c0
            got = _envs(p)
            assert int(got["episodes"].sum()) > 0
            for key in want:
                assert np.array_equal(got[key], want[key]), (mode, key)
            assert pol.get_rng() == want_rng == (9, 3 * inner * (reps + 1) if mode == "sample" else 0)      # fresh draws per replay
            p.close()
            pol.close()


def test_a_first_rollout_that_must_allocate_cannot_be_captured():
    import torch
    n = 128
    spec, params = seeded_policy((), "relu", None, seed=71)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        p = BatchedPropagator(default_config(4, GRAV_PM_J2), n, stream=side.cuda_stream)
        p.reset(sample_ic_batch(n, 4, seed=2))
        pol = P.DevicePolicy(spec, params)
        p.sync()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.BskError) as e:
                pol.rollout_device(p, 1, 1)
            assert e.value.code == -1 and "captured" in str(e.value)
        p.close()
        pol.close()


def test_step_policy_equals_step_tensors_on_the_policys_actions():
    import torch
    from basilisk_env_amd.envs.leoPowerAttitudeVecEnv import LeoPowerAttVecEnv
    n = 1000
    spec, params = _loop_policy((64, 64), (64, 64), 81)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        def make():
            probe = LeoPowerAttVecEnv(n, n_rw=4, step_duration=1.0, seed=3, device_reset_pool=128, device_sampler=True)
            cfg = probe.cfg
            probe.close()
            cfg.max_length = 6
            env = LeoPowerAttVecEnv(n, cfg=cfg, step_duration=1.0, seed=3, device_reset_pool=128, device_sampler=True, stream=side.cuda_stream)
            env.reset_tensors()
            return env
        e1, e2 = make(), make()
        pol1, pol2 = P.DevicePolicy(spec, params), P.DevicePolicy(spec, params)
        c0 = None
        for t in range(15):
            ob1, r1, d1, i1 = e1.step_policy(pol1)
            act = torch.from_dlpack(pol2.act(e2, "greedy", ("logp", "value"))["action"])
            ob2, r2, d2, i2 = e2.step_tensors(act)
            torch.cuda.synchronize()
            if t == 1:
                c0 = BatchedPropagator.debug_counters()
            assert i1["action"].dtype == torch.int32 and i1["logp"].dtype == torch.float32 and i1["value"].shape == (n,)
            assert torch.equal(i1["action"], act) and torch.equal(ob1, ob2) and torch.equal(r1, r2) and torch.equal(d1, d2)
            for key in i2:
                assert torch.equal(i1[key], i2[key]), key
        assert int(i1["episodes"].sum()) > 0 and len(set(i1["action"].tolist())) > 1
        # the loop itself is enqueue-only
        c0 = BatchedPropagator.debug_counters()
        for t in range(5):
            e1.step_policy(pol1, "sample")
        assert BatchedPropagator.debug_counters() == c0
        torch.cuda.synchronize()
        assert pol1.get_rng() == (0, 5)
        with pytest.raises(ValueError):
            e1.step_policy(pol1, "softmax")
        for x in (e1, e2, pol1, pol2):
            x.close()


def test_refusals_come_before_any_launch():
    import torch
    lib = _lib.load()
    spec, params = seeded_policy((16,), "relu", None, seed=91)
    pol = P.DevicePolicy(spec, params)
    spec_v, params_v = seeded_policy((16,), "relu", (16,), seed=91)
    pol_v = P.DevicePolicy(spec_v, params_v)
    n = 100
    obs = _device_obs(observation_like(n), 0)
    act = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    f32 = torch.full((3, n), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    h, o, a, f = pol._handle(), obs.data_ptr(), act.data_ptr(), f32.data_ptr()
    bad = [
        (None, o, n, n, 0, 0, a, None, None, None, 0, None),          # no policy
        (h, None, n, n, 0, 0, a, None, None, None, 0, None),          # no observations
        (h, o, n, n, 0, 0, None, None, None, None, 0, None),          # no actions
        (h, o, n, 0, 0, 0, a, None, None, None, 0, None),             # n < 1
        (h, o, n, -5, 0, 0, a, None, None, None, 0, None),
        (h, o, n - 1, n, 0, 0, a, None, None, None, 0, None),         # rows closer than n
        (h, o, n, n, -1, 0, a, None, None, None, 0, None),            # negative env_base
        (h, o, n, n, 0, 2, a, None, None, None, 0, None),             # bad mode
        (h, o, n, n, 0, -1, a, None, None, None, 0, None),
        (h, o, n, n, 0, 0, a, None, f, None, 0, None),                # value output without a value network
        (h, o, n, n, 0, 0, a, None, None, f, n - 1, None),            # logits rows closer than n
    ]
    for args in bad:
        assert lib.bsk_policy_act(*args) == -1, args
        assert lib.bsk_last_error()
    torch.cuda.synchronize()
    assert bool((act == -7).all()) and bool((f32 == -7).all())       # nothing was launched
    assert lib.bsk_policy_act(pol_v._handle(), o, n, n, 0, 0, a, None, f, None, 0, None) == 0
    torch.cuda.synchronize()
    assert bool((act != -7).all()) and bool((f32[0] != -7).all()) and bool((f32[1:] == -7).all())
    # rollout: NULL arguments, bad counts and modes, a value history without a value network
    prop = _stepped_propagator(n, steps=1)
    before = _envs(prop)
    hp = prop._handle()
    for args in ((None, hp, 0, 1, 1), (h, None, 0, 1, 1), (h, hp, 0, 0, 1), (h, hp, 0, 1, 0), (h, hp, 3, 1, 1)):
        assert lib.bsk_policy_rollout(*args, None, None, None, None, None, None) == -1, args
    assert lib.bsk_policy_rollout(h, hp, 0, 1, 1, None, None, None, None, None, f) == -1
    after = _envs(prop)
    for key in before:
        assert np.array_equal(before[key], after[key]), key
    # a policy and a handle on different devices
    if _hip.device_count() > 1:
        other = P.DevicePolicy(spec, params, device=1)
        assert lib.bsk_policy_rollout(other._handle(), hp, 0, 1, 1, None, None, None, None, None, None) == -1
        assert b"different devices" in lib.bsk_last_error()
        with pytest.raises(ValueError):
            other.act(prop)
        other.close()
    with pytest.raises(_lib.BskGpuUnavailable):
        P.DevicePolicy(spec, params, device=_hip.device_count())
    with pytest.raises(ValueError):
        pol.act(prop, "greedy", ("value",))
    with pytest.raises(ValueError):
        pol.act(prop, "greedy", ("entropy",))
    with pytest.raises(ValueError):
        pol.act(obs[:, ::2])
    with pytest.raises(ValueError):
        pol.act(obs.float())
    for x in (prop, pol, pol_v):
        x.close()


def test_c_consumer_closes_the_loop_like_the_python_binding(tmp_path):
    """tests/c_abi/c_abi_policy.c: bsk_policy_create + bsk_policy_rollout from plain C99 (no torch, no device allocator); its printout
    equals the Python binding's"""
    import os
    import subprocess
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "c_abi_policy"
    libdir = os.path.dirname(_lib.lib_path())
    subprocess.check_call(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-I", os.path.join(root_dir, "include"),
                           os.path.join(root_dir, "tests", "c_abi", "c_abi_policy.c"), "-L", libdir, "-lbskgpu",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    n = 150
    ic = sample_ic_batch(n, 4, seed=53)
    spec, params = _loop_policy((16,), (16,), 97)
    ic.tofile(tmp_path / "ic.bin")
    params.tofile(tmp_path / "params.bin")
    got = subprocess.check_output([str(exe), str(tmp_path / "ic.bin"), str(n), str(tmp_path / "params.bin")]).decode().split()
    prop = BatchedPropagator(default_config(4, GRAV_PM_J2), n)
    prop.reset(ic)
    prop.step(np.zeros(n, np.int32), 5)
    pol = P.DevicePolicy(spec, params)
    acts = pol.rollout(prop, 6, 5, "greedy")["action"]
    assert len(set(acts.ravel().tolist())) > 1
    o, r, _, _ = prop.get_obs()
    st = prop.get_state()
    rsum, _ = prop.batch_stats()
    want = [sum(o.ravel().tolist()), o[0, 0], r[n - 1], st[9, 1], rsum]
    assert [float(v) for v in got[:5]] == want
    pol.set_rng(123456789012345, 40)
    pol.rollout_device(prop, 3, 5, "sample")
    assert [int(v) for v in got[5:7]] == list(pol.get_rng()) == [123456789012345, 43]
    assert float(got[7]) == sum(prop.get_obs()[0].ravel().tolist())
    prop.close()
    pol.close()


def test_every_create_refuses_a_device_id_past_the_last_alike():
    """The admission of a device is written once (csrc/bsk_capi.hip: open_device) behind bsk_create, bsk_policy_create,
    bsk_population_create and bsk_es_create: BSK_ENODEV, *out left NULL and one text for all four.  Nothing is launched."""
    from helpers import create_each
    got = create_each(_hip.device_count(), hidden=(16,), n_members=2, n_envs=64)
    assert len(got) == 4
    for name, rc, out, text in got:
        assert rc == -2 and out is None and text == "device_id out of range", (name, rc, out, text)


def test_population_and_policy_rollouts_enqueue_the_same_loop():
    """The two rollouts share one per-step loop (csrc/bsk_capi_policy.hip: rollout_steps): a population of two members that both hold
    one policy's parameters leaves what that policy leaves on the same handle from the same reset, bit for bit - history rows and
    final handle state - with every history output given (the population's rows then come out of the fitness launch, the policy's out
    of the history launch) and with none given, no fitness output either (no third launch at all); and neither call copies or
    synchronises once a first one has allocated its scratch.  (tests/test_gpu_population.py holds a population of distinct members
    to separate policy rollouts on handles of E envs, all outputs given, and its rollout's host traffic in that configuration; the
    configuration without outputs, and the policy's side of the counters at this shape, are held here.)"""
    n, T, k = 128, 3, 2
    spec, params = _loop_policy((16,), (16,), 77)            # (the narrowest hidden layer there is)
    pol = P.DevicePolicy(spec, params)
    pop = P.PolicyPopulation(spec, np.stack([params, params]))
    prop = BatchedPropagator(default_config(4, GRAV_PM_J2), n)
    ic = sample_ic_batch(n, 4, seed=21)
    rows = (("obs", 40, np.float64, 5), ("reward", 8, np.float64, 1), ("reason", 1, np.uint8, 1), ("action", 4, np.int32, 1),
            ("logp", 4, np.float32, 1), ("value", 4, np.float32, 1))
    bufs = {key: _hip.DeviceBuffer(T * n * size, 0) for key, size, _, _ in rows}
    fit = {"d_env_value": _hip.DeviceBuffer(8 * n, 0), "d_env_len": _hip.DeviceBuffer(4 * n, 0), "d_fitness": _hip.DeviceBuffer(16, 0),
           "d_mean_len": _hip.DeviceBuffer(16, 0)}
    prop.reset(ic)
    pol.rollout_device(prop, 1, k, "greedy")               # (the first calls allocate the scratch rows)
    pop.rollout_device(prop, 1, k, "greedy")
    for given in (True, False):
        left = []
        for who in (pop, pol):
            prop.reset(ic)
            args = [bufs[key].ptr for key, _, _, _ in rows] if given else []
            kw = {key: b.ptr for key, b in fit.items()} if given and who is pop else {}
            c0 = BatchedPropagator.debug_counters()
            if who is pop:
                who.rollout_device(prop, T, k, "greedy", 0.97, *args, **kw)
            else:
                who.rollout_device(prop, T, k, "greedy", *args)
            assert BatchedPropagator.debug_counters() == c0, (given, who)       # no copy, no synchronisation
            prop.sync()
            hist = {key: _download(bufs[key].ptr, dt, T * n * m) for key, _, dt, m in rows} if given else {}
            left.append((hist, _envs(prop)))
        for part in (0, 1):
            assert set(left[0][part]) == set(left[1][part])
            for key in left[0][part]:
                a, b = left[0][part][key], left[1][part][key]
                assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (given, key)
        if given:
            assert len(set(left[0][0]["action"].tolist())) > 1              # (not a loop under one constant action)
    for x in list(bufs.values()) + list(fit.values()):
        x.free()
    for x in (prop, pol, pop):
        x.close()


def test_one_lifecycle_and_one_host_path_behind_the_three_bindings():
    """DevicePolicy, PolicyPopulation and DeviceEvolutionStrategy close through one base (basilisk_env_amd/policy.py: _DeviceObject):
    a second close is silent and a use after it is refused by name.  ``rollout`` and ``evaluate`` bring their results to the host
    through one helper (_ParamStore._host_rollout): what it returns equals what ``rollout_device`` leaves in buffers the caller owns,
    from the same state and the same seed.  The smallest shapes there are: one hidden layer of 16, 64 envs per member, two env steps
    of one substep."""
    T, k, E, members = 2, 1, 64, 2
    spec, params = _loop_policy((16,), (16,), 77)
    _, other = seeded_policy((16,), "relu", (16,), seed=78)
    pol = P.DevicePolicy(spec, params)
    pop = P.PolicyPopulation(spec, np.stack([params, other]))
    es = P.DeviceEvolutionStrategy(spec, params, members)
    # the policy: host rows against caller-owned device rows
    a, b = (_stepped_propagator(E, steps=1, k=k, seed=23) for _ in range(2))
    rows = (("obs", np.float64, 5), ("reward", np.float64, 1), ("reason", np.uint8, 1), ("action", np.int32, 1), ("logp", np.float32, 1),
            ("value", np.float32, 1))
    bufs = {key: _hip.DeviceBuffer(T * E * m * np.dtype(dt).itemsize, 0) for key, dt, m in rows}
    pol.set_rng(7, 3)
    host = pol.rollout(a, T, k, "sample")
    pol.set_rng(7, 3)
    pol.rollout_device(b, T, k, "sample", *(bufs[key].ptr for key, _, _ in rows))
    b.sync()
    assert list(host) == [key for key, _, _ in rows]
    for key, dt, m in rows:
        mine = _download(bufs[key].ptr, dt, T * E * m).reshape(host[key].shape)
        assert host[key].dtype == dt and host[key].tobytes() == mine.tobytes(), key
    assert pol.get_rng() == (7, 3 + T)
    # the population: host fitness against caller-owned device fitness
    n = members * E
    c, d = (_stepped_propagator(n, steps=1, k=k, seed=29) for _ in range(2))
    fit = (("env_value", np.float64, n), ("env_len", np.int32, n), ("fitness", np.float64, members), ("mean_len", np.float64, members))
    fbufs = {key: _hip.DeviceBuffer(count * np.dtype(dt).itemsize, 0) for key, dt, count in fit}
    pop.set_rng(9, 1)
    host = pop.evaluate(c, T, k, "sample", 0.97)
    pop.set_rng(9, 1)
    pop.rollout_device(d, T, k, "sample", 0.97, **{"d_" + key: fbufs[key].ptr for key, _, _ in fit})
    d.sync()
    assert list(host) == [key for key, _, _ in fit]
    for key, dt, count in fit:
        mine = _download(fbufs[key].ptr, dt, count)
        assert host[key].dtype == dt and host[key].shape == (count,) and host[key].tobytes() == mine.tobytes(), key
    assert np.all((host["env_len"] >= 1) & (host["env_len"] <= T)) and pop.get_rng() == (9, 1 + T)
    # the strategy: one launch into the population, then the wait all three inherit
    es.ask(pop)
    es.sync()
    assert np.array_equal(pop.member(0)[:10], params[:10]) and es.generation == 0
    for obj, what, use in ((pol, "policy", lambda: pol.get_rng()), (pop, "population", lambda: pop.member(0)),
                           (es, "evolution strategy", lambda: es.generation)):
        obj.close()
        obj.close()
        with pytest.raises(RuntimeError) as e:
            use()
        assert e.value.args == ("%s is closed" % what,)
        with pytest.raises(RuntimeError):
            obj._handle()
    for x in list(bufs.values()) + list(fbufs.values()):
        x.free()
    for x in (a, b, c, d):
        x.close()
