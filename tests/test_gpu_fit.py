"""GPU: the supervised fit of the device policy (bsk_fit_*; csrc/bsk_fit.hip; definition in include/bskgpu.h) and planner distillation
on top of it (planning.distill).

Output deltas go through the device library's expf and are held to the bound of tests/_fit_bounds.py against fp64.  Everything behind
them is an EQUALITY of bits for relu networks: the device's own deltas are handed to policy.fit_backward_ref / fit_accumulate_ref /
fit_step_ref as exact f32 numbers.  The accumulators A are read as Adam's first moment after one step with beta1 = 0, weight_decay = 0
and lr = 0: m = 0 * m + (1 - 0) * g = g = A / count exactly, and theta stays where it was.  tanh networks carry the derived bound.
Shapes are small: n = 65 is two blocks with one nearly empty, 200 is four with a tail, (128, 128, 128) is the widest network there
is.  The bit-for-bit cases go past every loop's first trip.  The fold (fit_fold_kernel) adds 32 blocks at a time and the rest one by
one: 2048 samples are one batch and no rest, 2049 one batch and a block of a single sample (a second time with one value target of
1e12, without which the f64 sum of f32 block gradients is exact in any order), 4400 + 100 two batches and five blocks
and then a second call onto a non-zero A - with a value network, so that the diagnostics row's value loss goes through the batched
loop too.  The weight gradients (fit_weight_grad) walk the wider side 64 rows at a time: (80, 48) and (112, 48) give a second trip
with 16 and 48 of its 64 lanes valid, in either orientation (the first layers, 80 and 112 over K = 5, own d_z rows; the second ones,
48 over K = 80 and K = 112, own h rows), a (96,) value network puts 96 rows over K = 5, (16, 128) puts 128 rows over K = 16 (two full
trips, 16 rows for the waves to split), (48, 112, 16) stacks three unequal hidden layers on the row offsets and the in-place deltas.
The two networks of a fit carry their own activations: both orders of tanh and relu are checked, each slice by the means its
activation allows.
"""
import subprocess

import numpy as np
import pytest

from _device_bits import build_c_consumer, download as _download, same as _same
from _fit_bounds import LEARNING, backward_bound, dlogits_bound, teacher_labels
from _policy_bounds import observation_like, seeded_policy, softmax_bound
from basilisk_env_amd import _lib, planning
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch

pytestmark = pytest.mark.gpu


def _batch(n, seed, masked=True):
    """observations, labels (some out of range) and alive bytes (some zero) for n samples, and the value targets"""
    rng = np.random.default_rng(300 + seed)
    obs = observation_like(n, seed)
    labels = rng.integers(0, 3, n).astype(np.int32)
    alive = np.ones(n, np.uint8)
    if masked and n > 8:
        labels[[2, n - 3]] = [3, -1]
        alive[[5, n // 2]] = 0
    return obs, labels, alive, rng.normal(size=n)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(view):
    """a device view (``__cuda_array_interface__``, dense) on the host"""
    cai = view.__cuda_array_interface__
    return _download(cai["data"][0], np.dtype(cai["typestr"]), int(np.prod(cai["shape"]))).reshape(cai["shape"])


class _Fit(object):
    """a policy with a fit attached, and one accumulate on host arrays -> the device's dlogits"""

    def __init__(self, spec, params, **kw):
        self.policy = P.DevicePolicy(spec, params)
        self.fit = P.PolicyFit(self.policy, **kw)

    def accumulate(self, obs, labels, alive=None, targets=None, stream=0):
        import torch
        n = obs.shape[1]
        self.d = [_dev(obs), _dev(labels), None if alive is None else _dev(alive), None if targets is None else _dev(targets),
                  torch.full((3, n), 7.0, dtype=torch.float32, device="cuda")]
        torch.cuda.synchronize()
        self.fit.accumulate(self.d[0], self.d[1], self.d[3], self.d[2], self.d[4], stream=stream)
        torch.cuda.synchronize()
        return self.d[4].cpu().numpy()

    def close(self):
        self.fit.close()
        self.policy.close()


NETS = {"relu16": ((16,), "relu"), "relu80_48": ((80, 48), "relu"), "tanh32": ((32,), "tanh")}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("net", sorted(NETS))
def test_output_deltas_lie_within_the_derived_bound(net, n):
    spec, params = seeded_policy(*NETS[net], seed=3)
    obs, labels, alive, _ = _batch(n, 1)
    f = _Fit(spec, params)
    got = f.accumulate(obs, labels, alive)
    g64, bound = dlogits_bound(spec, params, obs, labels, alive)
    err = np.abs(got.astype(np.float64) - g64)
    print("%s n=%d: max |device - fp64| %.3e, max bound %.3e, max ratio %.3f" % (net, n, err.max(), bound.max(), (err / np.maximum(bound, 1e-300))[bound > 0].max()))
    assert (err <= bound).all()
    off = bound[0] == 0
    assert n <= 8 or off.sum() == 4
    assert _same(got[:, off], np.zeros((3, int(off.sum())), np.float32))      # +0.0f, bit for bit
    row = f.fit.stats()
    assert row["count"] == int((~off).sum())
    f.close()


def _check_stats(row, spec, params, obs, labels, alive, targets):
    """The diagnostics row of a relu network against ``fit_stats_ref``: the logits and the value are the restatement's bit for bit, so
    the squared value error, the greedy choices and the count are EQUAL; the cross-entropy goes through the device library's expf and
    logf and lies within the sum of ``softmax_bound``'s bounds on the labels' log-probabilities."""
    ref = P.fit_stats_ref(spec, params, obs, labels, alive, targets)
    on = (labels >= 0) & (labels <= 2) & (alive != 0)
    assert row["count"] == ref[3] == on.sum() and row["correct"] == ref[2]
    assert _same(np.float64(row["value_loss_sum"]), np.float64(ref[1])) and (ref[1] > 0) == (targets is not None)
    _, _, logp64, _, e_logp = softmax_bound(P.mlp_ref(spec, params, obs)[0])
    pick = (np.clip(labels, 0, 2), np.arange(labels.size))
    want, tol = -logp64[pick][on].sum(), e_logp[pick][on].sum() * (1.0 + 2.0 ** -20)
    print("nll_sum: |device - fp64| %.3e, bound %.3e" % (abs(row["nll_sum"] - want), tol))
    assert abs(row["nll_sum"] - want) <= tol


def _reference_moment(spec, params, calls, value_coef):
    """A / count of the given accumulate calls [(obs, labels, alive, targets, device dlogits)], by the numpy restatements.  A sixth
    item is the d_dvalue the launch wrote (bsk_fit_accumulate_ppo): the device's own value deltas, taken as exact as dlogits is, in
    the place of the squared error's."""
    A, count = np.zeros(params.size), 0
    for call in calls:
        obs, labels, alive, targets, dl = call[:5]
        if len(call) > 5:
            dv = call[5]
        else:
            dv = None if targets is None else P.fit_dlogits32_ref(spec, params, obs, labels, alive, targets, value_coef)[1]
        G = P.fit_backward_ref(spec, params, obs, dl, dv)
        on = (labels >= 0) & (labels <= 2) & (alive != 0)
        A, count = P.fit_accumulate_ref(A, count, G, on.sum())
    z = np.zeros(params.size)
    return P.fit_step_ref(params.astype(np.float64), z, z, np.ones(2), 0, A, count, 0.0, 0.0, 0.999, 1e-8, 0.0)[1], count


BIT_CASES = {"relu16": ((16,), None, [200]), "relu128x3": ((128, 128, 128), None, [65]), "value": ((32, 16), (16,), [130]),
             "two_calls": ((16,), None, [100, 29]),
             # the fold past its batch of 32 blocks; the weight gradients past one trip of 64 rows (the module's docstring)
             "fold32": ((16,), None, [2048]), "fold33": ((16,), (16,), [2049]), "fold33_wide": ((16,), (16,), [2049]),
             "fold69_two_calls": ((16,), (16,), [4400, 100]),
             "w80_48": ((80, 48), None, [130]), "w112_48_v96": ((112, 48), (96,), [130]), "w16_128": ((16, 128), None, [130]),
             "w48_112_16": ((48, 112, 16), None, [65])}


@pytest.mark.parametrize("case", list(BIT_CASES))
def test_backward_and_accumulators_equal_the_restatement_bit_for_bit(case):
    hidden, vh, sizes = BIT_CASES[case]
    spec, params = seeded_policy(hidden, "relu", vh, seed=11)
    value_coef = 0.5
    f = _Fit(spec, params, lr=0.0, beta1=0.0, weight_decay=0.0, value_coef=value_coef)
    calls = []
    for k, n in enumerate(sizes):
        obs, labels, alive, targets = _batch(n, 20 + k)
        targets = targets if vh else None
        if case == "fold33_wide":
            # The f64 sum of a few dozen f32 block gradients of one magnitude is exact, whatever its order.  One target of 1e12
            # spreads the value network's block gradients over more than 53 bits: there the sum rounds, and the order shows.
            targets[n // 3] = 1e12
        dl = f.accumulate(obs, labels, alive, targets)
        calls.append((obs, labels, alive, targets, dl))
        _check_stats(f.fit.stats(), spec, params, obs, labels, alive, targets)
    f.fit.step()
    st = f.fit.state()
    want, count = _reference_moment(spec, params, calls, value_coef)
    assert count == sum(sizes) - 4 * len(sizes) and st["steps"] == 1
    assert np.count_nonzero(want) > want.size // 10 and not want[:10].any()
    assert _same(st["m"], want)
    assert _same(st["theta"], params.astype(np.float64))             # lr = 0: nothing moved
    f.close()


def test_tanh_backward_lies_within_the_derived_bound():
    spec, params = seeded_policy((32,), "tanh", seed=12)
    obs, labels, alive, _ = _batch(130, 31)
    f = _Fit(spec, params, lr=0.0, beta1=0.0, weight_decay=0.0)
    dl = f.accumulate(obs, labels, alive)
    f.fit.step()
    m = f.fit.state()["m"]
    count = f.fit.stats()["count"]
    G64, bound = backward_bound(spec, params, obs, dl)
    # (m * count is A up to the division's and the product's rounding: 2**-52 of |A| covers both)
    err, tol = np.abs(m * count - G64.sum(axis=0)), bound.sum(axis=0) * (1.0 + 2.0 ** -20) + 2.0 ** -52 * np.abs(G64.sum(axis=0))
    print("tanh (32,): max |A - fp64| %.3e, max bound %.3e, max ratio %.3f" % (err.max(), tol.max(), (err / np.maximum(tol, 1e-300)).max()))
    assert count == 126 and (err <= tol).all() and not m[:10].any()
    f.close()


@pytest.mark.parametrize("activation,value_activation", [("tanh", "relu"), ("relu", "tanh")])
def test_each_network_of_a_fit_runs_its_own_activation(activation, value_activation):
    """(32, 16) with a (48,) value network at n = 130, the two activations different.  The relu network's slice of A is the
    restatement's bit for bit whichever of the two it is; a tanh action network lies within ``backward_bound``; a tanh value network
    has no bound yet and is asked to be finite and NOT what the relu / relu restatement of the same floats gives.  Swapping the two
    activations changes both slices of the restatement, so a kernel that ran one network under the other's activation fails one
    of the two cases."""
    spec, params = seeded_policy((32, 16), activation, (48,), seed=19, value_activation=value_activation)
    relu_relu = P.check_spec((32, 16), "relu", (48,), "relu")
    value_coef = 0.5
    a_end = 10 + sum(o * i + o for o, i in P.layer_shapes(spec)[0])
    obs, labels, alive, targets = _batch(130, 33)
    f = _Fit(spec, params, lr=0.0, beta1=0.0, weight_decay=0.0, value_coef=value_coef)
    dl = f.accumulate(obs, labels, alive, targets)
    row = f.fit.stats()
    f.fit.step()
    st = f.fit.state()
    m = st["m"]
    calls = [(obs, labels, alive, targets, dl)]
    want, count = _reference_moment(spec, params, calls, value_coef)
    plain, _ = _reference_moment(relu_relu, params, calls, value_coef)
    swapped, _ = _reference_moment(P.check_spec((32, 16), value_activation, (48,), activation), params, calls, value_coef)
    assert row["count"] == count == 126 and st["steps"] == 1 and not m[:10].any() and 10 < a_end < m.size
    for lo, hi in ((10, a_end), (a_end, m.size)):
        assert np.count_nonzero(want[lo:hi]) > (hi - lo) // 10 and not _same(want[lo:hi], swapped[lo:hi])
    if activation == "relu":
        assert _same(m[10:a_end], want[10:a_end])
        assert np.isfinite(m[a_end:]).all() and np.count_nonzero(m[a_end:]) > (m.size - a_end) // 10
        assert not _same(m[a_end:], plain[a_end:])
    else:
        assert _same(m[a_end:], want[a_end:])
        assert _same(np.float64(row["value_loss_sum"]), np.float64(P.fit_stats_ref(spec, params, obs, labels, alive, targets)[1]))
        G64, bound = backward_bound(spec, params, obs, dl)
        G64, bound = G64.sum(axis=0)[10:a_end], bound.sum(axis=0)[10:a_end]
        # (m * count is A up to the division's and the product's rounding: 2**-52 of |A| covers both)
        err, tol = np.abs(m[10:a_end] * count - G64), bound * (1.0 + 2.0 ** -20) + 2.0 ** -52 * np.abs(G64)
        print("tanh (32, 16) over a relu value network: max |A - fp64| %.3e, max bound %.3e, max ratio %.3f"
              % (err.max(), tol.max(), (err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all()
    assert _same(st["theta"], params.astype(np.float64))             # lr = 0: nothing moved
    f.close()


def test_three_steps_equal_the_restatement_and_reach_the_policy():
    import torch
    spec, params = seeded_policy((32, 16), "relu", (16,), seed=13)
    kw = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-3)
    f = _Fit(spec, params, value_coef=0.5, **kw)
    a_end = 10 + sum(o * i + o for o, i in P.layer_shapes(spec)[0])
    state = (params.astype(np.float64), np.zeros(params.size), np.zeros(params.size), np.ones(2), 0)
    probe = observation_like(70, 9)
    for step in range(3):
        obs, labels, alive, targets = _batch(100, 40 + step)
        targets = targets if step == 1 else None                       # the value network moves in the second step alone
        now = state[0].astype(np.float32)                              # what the policy holds: (float)theta
        dl = f.accumulate(obs, labels, alive, targets)
        dv = None if targets is None else P.fit_dlogits32_ref(spec, now, obs, labels, alive, targets, 0.5)[1]
        G = P.fit_backward_ref(spec, now, obs, dl, dv)
        A, count = P.fit_accumulate_ref(np.zeros(params.size), 0, G, 96)
        f.fit.step()
        before = state
        state = P.fit_step_ref(*state, A, count, kw["lr"], kw["beta1"], kw["beta2"], kw["eps"], kw["weight_decay"],
                               n_update=None if step == 1 else a_end)[:5]
        got = f.fit.state()
        for k, name in enumerate(("theta", "m", "v", "beta_pow")):
            assert _same(got[name], state[k]), (step, name)
        assert got["steps"] == step + 1
        assert _same(got["theta"][:10], params[:10].astype(np.float64))                 # in_scale / in_shift never move
        if step != 1:                                                                   # without targets the value network stays
            assert all(_same(got[name][a_end:], before[k][a_end:]) for k, name in enumerate(("theta", "m", "v")))
        else:
            assert not np.array_equal(got["theta"][a_end:], before[0][a_end:])
        assert not np.array_equal(got["theta"][10:a_end], before[0][10:a_end])
        # the policy runs (float)theta
        res = f.policy.act(_dev(probe), want=("logits", "value"))
        torch.cuda.synchronize()
        l, v = P.mlp_ref(spec, state[0].astype(np.float32), probe)
        assert _same(_host(res["logits"]), l) and _same(_host(res["value"]), v)
    # a step with nothing accumulated moves nothing
    f.fit.step()
    got = f.fit.state()
    assert all(_same(got[name], state[k]) for k, name in enumerate(("theta", "m", "v", "beta_pow"))) and got["steps"] == 3
    # a checkpoint resumes: the state into a second fit, the same accumulate and step, the same bits
    g = _Fit(spec, params, value_coef=0.5, **kw)
    g.accumulate(*_batch(64, 51))                                      # (pending, with targets: set_state discards it)
    g.fit.set_state(got["theta"], got["m"], got["v"], got["beta_pow"], got["steps"])
    obs, labels, alive, _ = _batch(64, 50)
    for x in (f, g):
        x.accumulate(obs, labels, alive)
        x.fit.step()
    a, b = f.fit.state(), g.fit.state()
    assert all(_same(a[k], b[k]) for k in ("theta", "m", "v", "beta_pow")) and a["steps"] == b["steps"] == 4
    f.fit.lr = 0.5
    assert f.fit.lr == 0.5
    with pytest.raises(ValueError):
        f.fit.lr = -1.0
    f.close()
    g.close()


def test_a_fit_that_never_stepped_leaves_act_as_it_was():
    import torch
    spec, params = seeded_policy((32,), "tanh", (16,), seed=14)
    obs = _dev(observation_like(200, 4))
    plain = P.DevicePolicy(spec, params)
    f = _Fit(spec, params)
    f.accumulate(*_batch(100, 5)[:3])
    outs = []
    for pol in (plain, f.policy):
        pol.set_rng(7, 3)
        res = pol.act(obs, "sample")
        torch.cuda.synchronize()
        outs.append({k: _host(v) for k, v in res.items()})
    for k in ("action", "logp", "value", "logits"):
        assert _same(outs[0][k], outs[1][k]), k
    plain.close()
    f.close()


def test_accumulate_and_step_replay_from_a_hip_graph():
    import torch
    spec, params = seeded_policy((32,), "relu", (16,), seed=15)
    obs, labels, alive, targets = _batch(130, 60)
    side = torch.cuda.Stream()
    d = [_dev(obs), _dev(labels), _dev(targets), _dev(alive)]
    with torch.cuda.stream(side):
        eager, replayed, fresh = (_Fit(spec, params, lr=1e-2, weight_decay=1e-3) for _ in range(3))
        for _ in range(6):
            eager.fit.accumulate(*d, stream=side.cuda_stream)
            eager.fit.step(side.cuda_stream)
        # a first accumulate must allocate its scratch: refused under capture, and nothing is left half done
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            with pytest.raises(_lib.BskError) as e:
                fresh.fit.accumulate(*d, stream=side.cuda_stream)
            assert e.value.code == -1 and "captured" in str(e.value)
            fresh.fit.step(side.cuda_stream)                # (a step allocates nothing: capturable as it is)
        del graph
        # behind the one warming call a capture needs (it allocates the scratch) the pair is captured and replayed FIVE times:
        # iterations two to six of the eager run
        replayed.fit.accumulate(*d, stream=side.cuda_stream)
        replayed.fit.step(side.cuda_stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        c0 = BatchedPropagator.debug_counters()
        with torch.cuda.graph(graph, stream=side):
            replayed.fit.accumulate(*d, stream=side.cuda_stream)
            replayed.fit.step(side.cuda_stream)
        for _ in range(5):
            graph.replay()
        torch.cuda.synchronize()
        assert BatchedPropagator.debug_counters() == c0                # no copy, no synchronisation
        a, b = eager.fit.state(), replayed.fit.state()
        assert all(_same(a[k], b[k]) for k in ("theta", "m", "v", "beta_pow")) and a["steps"] == b["steps"] == 6
        assert eager.fit.stats() == replayed.fit.stats()
        del graph
        for x in (eager, replayed, fresh):
            x.close()


def test_the_device_fit_learns_the_teacher_rule():
    """the set-up tests/test_fit_host.py holds the reference alone to (``_fit_bounds.LEARNING``): teacher, network, seed, steps, lr"""
    spec, params = seeded_policy(LEARNING["hidden"], "relu", seed=LEARNING["seed"])
    obs = observation_like(256)
    labels = teacher_labels(obs)
    f = _Fit(spec, params, lr=LEARNING["lr"])
    d = [_dev(obs), _dev(labels)]
    rows = []
    for _ in range(LEARNING["steps"]):
        f.fit.accumulate(*d)
        rows.append(f.fit.stats())
        f.fit.step()
    f.fit.accumulate(*d)
    rows.append(f.fit.stats())
    first, last = rows[0], rows[-1]
    print("mean cross-entropy %.4f -> %.4f, correct %d -> %d of %d" % (first["nll_sum"] / 256, last["nll_sum"] / 256, first["correct"],
                                                                        last["correct"], last["count"]))
    assert first["count"] == last["count"] == 256
    assert last["nll_sum"] / 256 < 0.5 * first["nll_sum"] / 256
    assert last["correct"] >= first["correct"]
    f.close()


def _root(n, stream, seed=71):
    cfg = default_config(4, GRAV_PM_J2)
    cfg.max_length = 1000
    root = BatchedPropagator(cfg, n, stream=stream)
    root.reset(sample_ic_batch(n, 4, seed=seed))
    root.step(np.zeros(n, np.int32), 1)                     # (the observation buffers hold a step's output)
    return root


def _planner(kind, root):
    if kind == "beam":
        return planning.BeamPlanner(root, width=3, horizon=2, substeps=1)
    return planning.LookaheadPlanner(root, depth=1, substeps=1)


@pytest.mark.parametrize("kind,collect,value", [("lookahead", "expert", False), ("lookahead", "policy", False), ("beam", "expert", False),
                                                ("lookahead", "expert", True)])
def test_distillation_runs_on_the_device_end_to_end(kind, collect, value):
    import torch
    n, T = 64, 4
    spec, params = seeded_policy((16,), "relu", (16,), seed=16)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        root = _root(n, side.cuda_stream)
        planner = _planner(kind, root)
        f = _Fit(spec, params, lr=1e-2)
        planner.plan()                                      # (warming: whatever a first plan allocates)
        torch.cuda.synchronize()
        seen, wait = [], root.sync
        root.sync = lambda: (seen.append(BatchedPropagator.debug_counters()), wait())[1]
        c0 = BatchedPropagator.debug_counters()
        rows = planning.distill(planner, f.policy, f.fit, root, T, collect=collect, value_targets=value)
        root.sync = wait
        assert seen and seen[0] == c0                       # up to the one wait behind the loop: no copy, no synchronisation
        assert rows.shape == (T, 4) and (rows[:, 3] == n).all()         # every root alive at every step (no episode ends this early)
        assert np.isfinite(rows).all() and (rows[:, 0] > 0).all()
        assert ((rows[:, 1] > 0) == value).all()
        st = f.fit.state()
        a_end = 10 + sum(o * i + o for o, i in P.layer_shapes(spec)[0])
        assert st["steps"] == T and not np.array_equal(st["theta"][10:a_end], params[10:a_end].astype(np.float64))
        assert np.array_equal(st["theta"][a_end:], params[a_end:].astype(np.float64)) != value
        if collect == "expert":
            # the labels of every step: an identically seeded second root planned and stepped by hand
            root2 = _root(n, side.cuda_stream)
            planner2 = _planner(kind, root2)
            pol2 = P.DevicePolicy(spec, params)
            fit2 = P.PolicyFit(pol2, lr=1e-2)
            views = root2.device_views()
            for t in range(T):
                view = planner2.plan()
                labels = planner2.last_actions()
                fit2.accumulate(views["obs"], view, planner2.d_best_value.ptr if value else None, stream=side.cuda_stream)
                row = fit2.stats()
                assert [row["nll_sum"], row["value_loss_sum"], row["correct"], row["count"]] == rows[t].tolist(), t
                assert ((labels >= 0) & (labels <= 2)).all()
                root2.step_device(view.__cuda_array_interface__["data"][0], 1)
                fit2.step(side.cuda_stream)
            assert np.array_equal(root.get_state(), root2.get_state())
            assert all(_same(st[k], fit2.state()[k]) for k in ("theta", "m", "v"))
            for x in (fit2, pol2, planner2, root2):
                x.close()
        for x in (f, planner, root):
            x.close()


def test_roots_that_end_inside_the_loop_stop_contributing():
    """Episodes of 5 env steps on an auto-resetting root whose step counters are staggered by hand, so that roots end at
    different steps of the loop and start again: the count of every step's row is the number of roots with no reason byte so far in
    the loop, counted by hand on a second root stepped step by step; a root that ended stays out once its next episode runs; and
    the fit ends in the bits of a hand-made loop that passes the same mask."""
    import torch
    n, T = 64, 6
    spec, params = seeded_policy((16,), "relu", seed=18)
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    cfg.max_length = 5
    ic, pool = sample_ic_batch(n, 4, seed=72), sample_ic_batch(23, 4, seed=73)
    side = torch.cuda.Stream()

    def root():
        r = BatchedPropagator(cfg, n, stream=side.cuda_stream)
        r.set_ic_pool(pool)
        r.reset(ic)
        r.step(np.zeros(n, np.int32), 1)
        steps, ticks = r.get_counters()
        r.set_counters(steps + np.arange(n, dtype=np.int32) % 4, ticks)          # a quarter of the episodes ends at each of four steps
        return r

    with torch.cuda.stream(side):
        r1, r2 = root(), root()
        p1, p2 = _planner("lookahead", r1), _planner("lookahead", r2)
        f, g = _Fit(spec, params, lr=1e-2), _Fit(spec, params, lr=1e-2)
        rows = planning.distill(p1, f.policy, f.fit, r1, T)
        # by hand: plan, accumulate under the mask kept on the host, step, fit step
        views = r2.device_views()
        alive, counts, came_back = np.ones(n, bool), [], 0
        for t in range(T):
            view = p2.plan()
            d_alive = _dev(alive.astype(np.uint8))
            torch.cuda.synchronize()
            g.fit.accumulate(views["obs"], view, None, d_alive, stream=side.cuda_stream)
            row = g.fit.stats()
            counts.append(int(alive.sum()))
            assert [row["nll_sum"], row["value_loss_sum"], row["correct"], row["count"]] == rows[t].tolist(), t
            r2.step_device(view.__cuda_array_interface__["data"][0], 1)
            g.fit.step(side.cuda_stream)
            reason = r2.get_obs()[3]
            came_back += int((~alive & (reason == 0)).sum())                         # ended earlier, running again: still out
            alive &= reason == 0
        assert rows[:, 3].tolist() == counts
        # (which step ends an episode is the env's business: what is asked is that roots end at several steps, and some run again)
        assert counts[0] == n and counts == sorted(counts, reverse=True) and len(set(counts)) >= 3 and counts[-1] < n // 2 and came_back > 0
        a, b = f.fit.state(), g.fit.state()
        assert all(_same(a[k], b[k]) for k in ("theta", "m", "v", "beta_pow")) and a["steps"] == b["steps"]
        assert a["steps"] == sum(c > 0 for c in counts)
        assert np.array_equal(r1.get_state(), r2.get_state())
        for x in (f, g, p1, p2, r1, r2):
            x.close()


def test_c_consumer_prints_the_python_bindings_fit(tmp_path):
    """tests/c_abi/c_abi_fit.c: bsk_fit_create / _accumulate / _step / _stats_device / _get_state from plain C99; its hex-float printout
    equals the Python binding's"""
    exe = build_c_consumer(tmp_path, "c_abi_fit")
    n = 100
    spec, params = seeded_policy((16,), "relu", seed=17)
    obs, labels, _, _ = _batch(n, 80)
    params.tofile(tmp_path / "params.bin")
    np.ascontiguousarray(obs).tofile(tmp_path / "obs.bin")
    labels.tofile(tmp_path / "labels.bin")
    got = subprocess.check_output([str(exe)] + [str(tmp_path / x) for x in ("params.bin", "obs.bin", "labels.bin")] + [str(n)]).decode().split()
    f = _Fit(spec, params, lr=1e-2, weight_decay=1e-3)
    f.accumulate(obs, labels)
    row = f.fit.stats()
    f.fit.step()
    st = f.fit.state()
    want = [row["nll_sum"], row["value_loss_sum"], float(row["correct"]), float(row["count"])] + st["theta"][10:14].tolist() + \
           [float(st["steps"])] + st["beta_pow"].tolist()
    assert [float.fromhex(x) for x in got] == want
    assert want[3] == 98.0 and want[8] == 1.0 and st["theta"][10] != float(params[10])
    f.close()
