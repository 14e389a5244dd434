"""GPU: policy-gradient training on the device - bsk_gae, bsk_fit_accumulate_pg (csrc/bsk_fit.hip: gae_kernel, fit_block_kernel<true>;
definition in include/bskgpu.h) and the loop ``policy.PolicyGradient`` over them.

bsk_gae is f64 additions and products with no library function: EQUAL to ``gae_ref`` in every bit.  The output deltas go through the
device library's expf and logf and are held to the bound of tests/_pg_bounds.py against the fp64 formula on the device's OWN f32
logits (``bsk_policy_act``'s, which the fit's forward pass repeats bit for bit).  Everything behind the deltas is
tests/test_gpu_fit.py's equality of bits for relu networks, by the same reading of the accumulators A through Adam's first moment
(beta1 = 0, lr = 0).  Shapes are the smallest at which each loop goes past its first trip: 65 samples are two blocks, 200 four with a
tail, 2049 a fold batch of 32 blocks plus one; n_envs = 300 is two workgroups of the estimator, n_steps = 7 several trips of its loop.
"""
import numpy as np
import pytest

from _device_bits import download as _download, same as _same
from _fit_bounds import teacher_labels
from _pg_bounds import LEARNING_PG, pg_dlogits_bound, pg_inputs, pg_stats_bound
from _policy_bounds import observation_like, seeded_policy
from basilisk_env_amd import _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from test_gpu_fit import NETS, _batch, _dev, _host, _reference_moment
from test_pg_host import gae_case

pytestmark = pytest.mark.gpu

EINVAL = -1


# ------------------------------------------------------------------------------------------------------------------ bsk_gae
@pytest.mark.parametrize("n_envs", [1, 64, 65, 300])
@pytest.mark.parametrize("n_steps", [1, 2, 7])
def test_gae_equals_the_restatement_bit_for_bit(n_steps, n_envs):
    import torch
    T, N, stride, g, lam = n_steps, n_envs, n_envs + 3, 0.97, 0.9
    reward, reason, value, last = gae_case(T, N, seed=T)

    def padded(a, fill):
        out = np.full((T, stride), fill, a.dtype)
        out[:, :N] = a
        return _dev(out)
    d_reward, d_reason, d_value, d_last = padded(reward, 9.0), padded(reason, 0), padded(value, 9.0), _dev(last)
    for with_last in (False, True):
        for with_ret in (False, True):
            adv = torch.full((T, stride), -7.0, dtype=torch.float32, device="cuda")
            ret = torch.full((T, stride), -7.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            P.gae(d_reward, d_reason, d_value, d_last if with_last else None, T, N, adv, ret if with_ret else None, g, lam, stride=stride)
            torch.cuda.synchronize()
            want_adv, want_ret = P.gae_ref(reward, reason, value, last if with_last else None, g, lam)
            got_adv, got_ret = adv.cpu().numpy(), ret.cpu().numpy()
            assert _same(got_adv[:, :N], want_adv), (with_last, with_ret)
            assert _same(got_ret[:, :N], want_ret if with_ret else np.full((T, N), -7.0)), (with_last, with_ret)
            assert (got_adv[:, N:] == -7.0).all() and (got_ret[:, N:] == -7.0).all()         # the padding is nobody's
    if T > 1 and N > 3:
        assert not _same(*[P.gae_ref(reward, reason, value, x, g, lam)[0] for x in (None, last)])


def test_gae_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    import torch
    T, N = 2, 5
    lib = _lib.load()
    reward, reason, value, last = (_dev(a) for a in gae_case(T, N))
    adv = torch.full((T, N), -7.0, dtype=torch.float32, device="cuda")
    ret = torch.full((T, N), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    good = [vp(reward), vp(reason), vp(value), vp(last), T, N, N, 0.9, 0.9, vp(adv), vp(ret), None]
    nan, inf = float("nan"), float("inf")
    for at, bad in ((0, None), (1, None), (2, None), (9, None), (4, 0), (5, 0), (6, N - 1), (7, -0.1), (7, 1.1), (7, nan), (8, -0.1), (8, 1.1),
                    (8, inf), (8, nan)):
        args = list(good)
        args[at] = bad
        assert lib.bsk_gae(*args) == EINVAL, (at, bad)
    torch.cuda.synchronize()
    assert (adv.cpu().numpy() == -7.0).all() and (ret.cpu().numpy() == -7.0).all()
    assert lib.bsk_gae(*good) == 0
    torch.cuda.synchronize()
    assert _same(adv.cpu().numpy(), P.gae_ref(*[t.cpu().numpy() for t in (reward, reason, value, last)], 0.9, 0.9)[0])
    with pytest.raises(ValueError):
        P.gae(reward, reason, value, None, T, N, adv, gamma=1.5)


# ------------------------------------------------------------------------------------------------------------------ the deltas
class _PG(object):
    """a policy with a fit attached, and one accumulate_pg on host arrays -> the device's dlogits"""

    def __init__(self, spec, params, **kw):
        self.spec, self.params = spec, params
        self.policy = P.DevicePolicy(spec, params)
        self.fit = P.PolicyFit(self.policy, **kw)

    def logits(self, obs):
        """the device's own f32 logits (3, n)"""
        import torch
        res = self.policy.act(_dev(obs), want=("logits",))
        torch.cuda.synchronize()
        return _host(res["logits"])

    def accumulate_pg(self, obs, actions, adv, old=None, clip=0.2, ent_coef=0.0, alive=None, targets=None, stream=0):
        import torch
        n = obs.shape[1]
        opt = lambda a: None if a is None else _dev(a)      # noqa: E731
        self.d = [_dev(obs), _dev(actions), _dev(adv), opt(old), opt(targets), opt(alive),
                  torch.full((3, n), 7.0, dtype=torch.float32, device="cuda")]
        torch.cuda.synchronize()
        self.fit.accumulate_pg(self.d[0], self.d[1], self.d[2], self.d[3], clip, ent_coef, self.d[4], self.d[5], self.d[6], stream=stream)
        torch.cuda.synchronize()
        return self.d[6].cpu().numpy()

    def accumulate(self, obs, labels, alive=None, targets=None):
        import torch
        n = obs.shape[1]
        opt = lambda a: None if a is None else _dev(a)      # noqa: E731
        self.d = [_dev(obs), _dev(labels), opt(targets), opt(alive), torch.full((3, n), 7.0, dtype=torch.float32, device="cuda")]
        torch.cuda.synchronize()
        self.fit.accumulate(*self.d)
        torch.cuda.synchronize()
        return self.d[4].cpu().numpy()

    def close(self):
        self.fit.close()
        self.policy.close()


def _lp_of(logits, actions):
    """fp64 log-probabilities of ``actions`` (clipped into range) from logits (3, n)"""
    l = logits.astype(np.float64)
    z = l - l.max(axis=0)
    return (z - np.log(np.exp(z).sum(axis=0)))[np.clip(actions, 0, 2), np.arange(l.shape[1])]


def pg_case(f, n, seed, ppo=True):
    """``test_gpu_fit._batch``'s observations, masked labels (as actions) and alive bytes; advantages N(0, 1) with exact zeros; old
    log-probabilities lp_a + N(0, 0.3**2) from the device's own logits -> (obs, actions, alive, targets, adv, old, logits)"""
    obs, actions, alive, targets = _batch(n, seed)
    logits = f.logits(obs)
    adv, old = pg_inputs(n, seed, _lp_of(logits, actions) if ppo else None)
    return obs, actions, alive, targets, adv, old, logits


@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("net", sorted(NETS))
def test_pg_output_deltas_lie_within_the_derived_bound(net, n, ent_coef):
    """PPO mode, clip = 0.2: with old log-probabilities 0.3 away (one sigma) a good share of the samples lies beyond either edge.  A
    sample whose fp64 ratio lies within the bound on r of an edge is left out - the device may gate it either way - and at most
    one in a hundred may be (with these seeds, on the restatement's logits: none)."""
    clip = 0.2
    spec, params = seeded_policy(*NETS[net], seed=3)
    f = _PG(spec, params)
    obs, actions, alive, _, adv, old, logits = pg_case(f, n, 1)
    if NETS[net][1] == "relu":
        assert _same(logits, P.mlp_ref(spec, params, obs)[0])
    got = f.accumulate_pg(obs, actions, adv, old, clip, ent_coef, alive)
    on = (actions >= 0) & (actions <= 2) & (alive != 0)
    b = pg_dlogits_bound(logits, actions, adv, old, clip, ent_coef, on)
    use = ~b["band"]
    err = np.abs(got.astype(np.float64) - b["g"])
    ratio = (err / np.maximum(b["bound"], 1e-300))[:, on & use]
    print("%s n=%d ent=%g: max |device - fp64| %.3e, max bound %.3e, max ratio %.3f, in the band %d, clipped %d of %d"
          % (net, n, ent_coef, err[:, use].max(), b["bound"].max(), ratio.max() if ratio.size else 0.0, b["band"].sum(),
             b["terms"]["clipped"][on].sum(), on.sum()))
    assert b["band"].sum() * 100 <= n
    assert (err[:, use] <= b["bound"][:, use]).all()
    assert n <= 8 or (~on).sum() == 4
    assert _same(got[:, ~on], np.zeros((3, int((~on).sum())), np.float32))      # +0.0f, bit for bit
    if n >= 63:
        r, A = b["terms"]["r"][on], adv[on]
        assert ((r > 1.2) & (A > 0)).sum() >= 2 and ((r < 0.8) & (A < 0)).sum() >= 2 and (A == 0).sum() >= 1
    # the two rows: counts are equal, sums lie within the summed per-sample bounds
    row, pg = f.fit.stats(), f.fit.pg_stats()
    assert row["count"] == on.sum()
    want, tol = pg_stats_bound(b, on)
    free = int((b["band"] & on).sum())
    assert want[2] <= pg["clipped"] <= want[2] + free
    if free == 0:
        got_row = np.array([pg["kl_sum"], pg["entropy_sum"], pg["clipped"], pg["surrogate_sum"]])
        print("pg row: |device - fp64| %s, bound %s" % (np.abs(got_row - want), tol))
        assert (np.abs(got_row - want) <= tol).all()
        if NETS[net][1] == "relu":
            assert pg["clipped"] == P.fit_pg_stats_ref(spec, params, obs, actions, adv, old, clip, alive)[2]
    f.close()


PG_BIT_CASES = {"relu16": ((16,), None, [200]), "relu80_48": ((80, 48), None, [130]), "value": ((32, 16), (16,), [130]),
                "two_calls": ((16,), None, [100, 29]), "fold33": ((16,), (16,), [2049])}


@pytest.mark.parametrize("case", list(PG_BIT_CASES))
def test_pg_backward_and_accumulators_equal_the_restatement_bit_for_bit(case):
    hidden, vh, sizes = PG_BIT_CASES[case]
    spec, params = seeded_policy(hidden, "relu", vh, seed=11)
    value_coef = 0.5
    f = _PG(spec, params, lr=0.0, beta1=0.0, weight_decay=0.0, value_coef=value_coef)
    calls = []
    for k, n in enumerate(sizes):
        obs, actions, alive, targets, adv, old, _ = pg_case(f, n, 20 + k)
        targets = targets if vh else None
        dl = f.accumulate_pg(obs, actions, adv, old, 0.2, 0.01, alive, targets)
        calls.append((obs, actions, alive, targets, dl))
        on = (actions >= 0) & (actions <= 2) & (alive != 0)
        ref = P.fit_stats_ref(spec, params, obs, actions, alive, targets)
        row = f.fit.stats()
        assert row["count"] == ref[3] == on.sum() and row["correct"] == ref[2] and _same(np.float64(row["value_loss_sum"]), np.float64(ref[1]))
    f.fit.step()
    st = f.fit.state()
    want, count = _reference_moment(spec, params, calls, value_coef)
    assert count == sum(sizes) - 4 * len(sizes) and st["steps"] == 1
    assert np.count_nonzero(want) > want.size // 10 and not want[:10].any()
    assert _same(st["m"], want)
    assert _same(st["theta"], params.astype(np.float64))             # lr = 0: nothing moved
    f.close()


def test_a_supervised_and_a_pg_accumulate_add_into_one_accumulator():
    spec, params = seeded_policy((16,), "relu", seed=11)
    f = _PG(spec, params, lr=0.0, beta1=0.0, weight_decay=0.0)
    obs, labels, alive, _ = _batch(100, 25)
    calls = [(obs, labels, alive, None, f.accumulate(obs, labels, alive))]
    obs, actions, alive, _, adv, old, _ = pg_case(f, 70, 26)
    calls.append((obs, actions, alive, None, f.accumulate_pg(obs, actions, adv, old, 0.2, 0.01, alive)))
    f.fit.step()
    st = f.fit.state()
    want, count = _reference_moment(spec, params, calls, 0.0)
    assert count == 162 and st["steps"] == 1 and _same(st["m"], want) and np.count_nonzero(want) > want.size // 10
    f.close()


# ------------------------------------------------------------------------------------------------------------------ what follows from the definition
@pytest.mark.parametrize("vh", [None, (16,)])
def test_unit_advantages_without_a_ratio_are_the_supervised_accumulate_bit_for_bit(vh):
    spec, params = seeded_policy((32, 16), "relu", vh, seed=21)
    obs, labels, alive, targets = _batch(200, 27)
    targets = targets if vh else None
    a = _PG(spec, params, lr=0.0, beta1=0.0, weight_decay=0.0)
    b = _PG(spec, params, lr=0.0, beta1=0.0, weight_decay=0.0)
    da = a.accumulate(obs, labels, alive, targets)
    db = b.accumulate_pg(obs, labels, np.ones(200, np.float32), None, 0.2, 0.0, alive, targets)
    assert _same(da, db) and np.count_nonzero(da) == 3 * 196
    ra, rb = a.fit.stats(), b.fit.stats()
    assert all(_same(np.float64(ra[k]), np.float64(rb[k])) for k in ("value_loss_sum", "correct", "count")) and rb["count"] == 196
    # (the cross-entropy column goes through logf in either kernel's own form: equal to rounding, not to the bit)
    assert abs(ra["nll_sum"] - rb["nll_sum"]) <= 196 * 2.0 ** -21 and (ra["value_loss_sum"] > 0) == (vh is not None)
    pg = b.fit.pg_stats()
    assert _same(np.float64(pg["kl_sum"]), np.float64(0.0)) and pg["clipped"] == 0 and pg["surrogate_sum"] == 196.0 and pg["entropy_sum"] > 0
    for x in (a, b):
        x.fit.step()
    sa, sb = a.fit.state(), b.fit.state()
    assert _same(sa["m"], sb["m"]) and np.count_nonzero(sa["m"]) > sa["m"].size // 10 and sa["steps"] == sb["steps"] == 1
    a.close()
    b.close()


def _block_sum(x):
    """sample-ascending within blocks of 64 from +0.0, then block-ascending from +0.0: the order of the diagnostics rows"""
    total = 0.0
    for b in range(0, x.size, 64):
        part = 0.0
        for v in x[b:b + 64].astype(np.float64).tolist():
            part = part + v
        total = total + part
    return total


@pytest.mark.parametrize("net", ["relu80_48", "tanh32"])
def test_old_log_probabilities_of_the_policy_itself_give_ratio_one(net):
    """logp_old straight from bsk_policy_act in sample mode, parameters unchanged: lp_a is formed as policy_kernel forms logp, so d
    is +0.0f for every sample - the KL column is 0.0, nothing is clipped, and the surrogate column is the sum of A exactly."""
    import torch
    n = 200
    spec, params = seeded_policy(*NETS[net], seed=5)
    f = _PG(spec, params)
    obs = observation_like(n, 3)
    adv = pg_inputs(n, 3)[0]
    d_obs, d_adv = _dev(obs), _dev(adv)
    f.policy.set_rng(11, 4)
    res = f.policy.act(d_obs, "sample", want=("logp",))
    torch.cuda.synchronize()
    actions = _host(res["action"])
    assert min(np.bincount(actions, minlength=3)) >= 5
    f.fit.accumulate_pg(d_obs, res["action"], d_adv, res["logp"], 0.2, 0.01)
    pg = f.fit.pg_stats()
    assert _same(np.float64(pg["kl_sum"]), np.float64(0.0)) and pg["clipped"] == 0
    assert _same(np.float64(pg["surrogate_sum"]), np.float64(_block_sum(adv)))
    assert f.fit.stats()["count"] == n
    f.close()


def test_zero_advantages_contribute_zero_deltas_and_are_counted():
    spec, params = seeded_policy((16,), "relu", seed=6)
    f = _PG(spec, params, lr=0.0, beta1=0.0, weight_decay=0.0)
    n = 130
    obs, actions, alive, _, adv, old, _ = pg_case(f, n, 28)
    adv[::3] = 0.0
    on = (actions >= 0) & (actions <= 2) & (alive != 0)
    for o in (None, old):
        got = f.accumulate_pg(obs, actions, adv, o, 0.2, 0.0, alive)
        zero = on & (adv == 0)
        assert zero.sum() > 40 and _same(got[:, zero], np.zeros((3, int(zero.sum())), np.float32))
        assert f.fit.stats()["count"] == on.sum() == n - 4
    # all advantages zero: the step counts the samples and the mean gradient is +0.0 in every bit
    f.fit.step()
    g = _PG(spec, params, lr=0.0, beta1=0.0, weight_decay=0.0)
    got = g.accumulate_pg(obs, actions, np.zeros(n, np.float32), old, 0.2, 0.0, alive)
    assert _same(got, np.zeros((3, n), np.float32)) and g.fit.stats()["count"] == n - 4
    g.fit.step()
    st = g.fit.state()
    assert st["steps"] == 1 and _same(st["m"], np.zeros(params.size))
    # ... and with an entropy bonus they carry the bonus's gradient alone
    got = g.accumulate_pg(obs, actions, np.zeros(n, np.float32), old, 0.2, 0.01, alive)
    assert got[:, on].all()
    f.close()
    g.close()


def test_pg_argument_rules_on_the_device():
    import ctypes as C
    spec, params = seeded_policy((16,), "relu", seed=6)
    f = _PG(spec, params)
    obs, actions, alive, _, adv, old, _ = pg_case(f, 70, 29)
    dl = f.accumulate_pg(obs, actions, adv, old, 0.2, 0.01, alive)
    row, pg = f.fit.stats(), f.fit.pg_stats()
    lib, h = _lib.load(), f.fit._handle()
    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    d = f.d
    good = [h, vp(d[0]), 70, 70, vp(d[1]), vp(d[2]), vp(d[3]), 0.2, 0.01, None, vp(d[5]), vp(d[6]), 70, None]
    nan, inf = float("nan"), float("inf")
    for at, bad in ((0, None), (1, None), (4, None), (5, None), (7, 0.0), (7, 1.0), (7, nan), (7, inf), (8, -0.1), (8, nan), (8, inf), (3, 0),
                    (2, 69), (12, 69), (9, vp(d[2]))):
        args = list(good)
        args[at] = bad
        assert lib.bsk_fit_accumulate_pg(*args) == EINVAL, (at, bad)
    # clip is not read without old log-probabilities
    args = list(good)
    args[6], args[7] = None, 7.0
    assert lib.bsk_fit_accumulate_pg(*args) == 0
    assert lib.bsk_fit_accumulate_pg(*good) == 0
    import torch
    torch.cuda.synchronize()
    assert f.fit.stats() == row and f.fit.pg_stats() == pg and _same(d[6].cpu().numpy(), dl)
    with pytest.raises(ValueError):
        f.fit.accumulate_pg(d[0], d[1], d[2], d[3], clip=1.0)
    with pytest.raises(ValueError):
        f.fit.accumulate_pg(d[0], d[1], None)
    with pytest.raises(ValueError):
        f.fit.accumulate_pg(d[0], d[1], d[2][:5])
    f.close()


# ------------------------------------------------------------------------------------------------------------------ capture
def test_gae_accumulate_pg_and_step_replay_from_a_hip_graph():
    import torch
    T, n = 2, 130
    spec, params = seeded_policy((32,), "relu", (16,), seed=15)
    obs, actions, alive, _ = _batch(n, 60)
    reward, reason, value, last = gae_case(T, n, seed=3)
    actions = np.clip(actions, 0, 2)
    l = P.mlp_ref(spec, params, obs)[0]
    old = (_lp_of(l, actions) + np.random.default_rng(61).normal(0.0, 0.3, n)).astype(np.float32)
    side = torch.cuda.Stream()
    d = {k: _dev(v) for k, v in dict(obs=obs, actions=actions, alive=alive, reward=reward, reason=reason, value=value, last=last, old=old).items()}
    with torch.cuda.stream(side):
        eager, replayed = (_PG(spec, params, lr=1e-2, weight_decay=1e-3) for _ in range(2))
        bufs = [(torch.zeros((T, n), dtype=torch.float32, device="cuda"), torch.zeros((T, n), dtype=torch.float64, device="cuda")) for _ in range(2)]

        def launches(x, adv, ret):
            P.gae(d["reward"], d["reason"], d["value"], d["last"], T, n, adv, ret, 0.97, 0.9, stream=side.cuda_stream)
            x.fit.accumulate_pg(d["obs"], d["actions"], adv[0], d["old"], 0.2, 0.01, ret[0], d["alive"], stream=side.cuda_stream)
            x.fit.step(side.cuda_stream)
        for _ in range(3):
            launches(eager, *bufs[0])
        launches(replayed, *bufs[1])                       # (warming: the first accumulate allocates the scratch)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        c0 = BatchedPropagator.debug_counters()
        with torch.cuda.graph(graph, stream=side):
            launches(replayed, *bufs[1])
        for _ in range(2):
            graph.replay()
        torch.cuda.synchronize()
        assert BatchedPropagator.debug_counters() == c0                # no copy, no synchronisation
        a, b = eager.fit.state(), replayed.fit.state()
        assert all(_same(a[k], b[k]) for k in ("theta", "m", "v", "beta_pow")) and a["steps"] == b["steps"] == 3
        assert not np.array_equal(a["theta"], params.astype(np.float64))
        assert eager.fit.stats() == replayed.fit.stats() and eager.fit.pg_stats() == replayed.fit.pg_stats()
        assert eager.fit.pg_stats()["kl_sum"] != 0.0
        assert all(_same(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(*bufs))
        assert _same(bufs[0][0].cpu().numpy(), P.gae_ref(reward, reason, value, last, 0.97, 0.9)[0])
        del graph
        eager.close()
        replayed.close()


# ------------------------------------------------------------------------------------------------------------------ learning
def test_the_device_learns_the_bandit():
    """``_pg_bounds.LEARNING_PG`` on the device: actions sampled by bsk_policy_act, rewards formed here on the host, A2C mode.  The
    greedy agreement with the teacher reaches the midpoint between the recorded initial agreement and the recorded lowest final one
    of the restatement: half the reference's own improvement (a draw within expf's error of a probability boundary may pick another
    action than numpy, so the trajectories are not comparable bit for bit)."""
    import torch
    L = LEARNING_PG
    spec, params = seeded_policy(L["hidden"], "relu", seed=L["seed"])
    obs = observation_like(256)
    teacher = teacher_labels(obs)
    f = _PG(spec, params, lr=L["lr"])
    d_obs = _dev(obs)

    def agreement():
        res = f.policy.act(d_obs, "greedy", want=())
        torch.cuda.synchronize()
        return int((_host(res["action"]) == teacher).sum())
    first = agreement()
    assert first == L["initial"]
    f.policy.set_rng(0, 0)
    for _ in range(L["steps"]):
        res = f.policy.act(d_obs, "sample", want=())
        torch.cuda.synchronize()
        adv = _dev((_host(res["action"]) == teacher).astype(np.float32) - np.float32(0.5))
        torch.cuda.synchronize()
        f.fit.accumulate_pg(d_obs, res["action"], adv)
        f.fit.step()
    last = agreement()
    print("greedy agreement with the teacher: %d -> %d of 256 (the restatement alone: %d -> at least %d)" % (first, last, L["initial"], L["final_min"]))
    assert 2 * last >= L["initial"] + L["final_min"]
    f.close()


# ------------------------------------------------------------------------------------------------------------------ the loop
def test_policy_gradient_runs_on_the_device_end_to_end():
    import torch
    n, T = 256, 8
    spec, params = seeded_policy((16,), "relu", (16,), seed=16)
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_AUTO_RESET
    cfg.max_length = 5                                      # (episodes end, and start again, inside every rollout)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        root = BatchedPropagator(cfg, n, stream=side.cuda_stream)
        root.set_ic_pool(sample_ic_batch(23, 4, seed=73))
        root.reset(sample_ic_batch(n, 4, seed=72))
        root.step(np.zeros(n, np.int32), 1)                 # (the observation buffers hold a step's output)
        steps, ticks = root.get_counters()
        root.set_counters(steps + np.arange(n, dtype=np.int32) % 4, ticks)          # episodes end at different steps
        f = _PG(spec, params, lr=1e-2)
        with pytest.raises(ValueError):
            plain = BatchedPropagator(default_config(4, GRAV_PM_J2), 64, stream=side.cuda_stream)
            try:
                P.PolicyGradient(plain, f.policy, f.fit, T)
            finally:
                plain.close()
        pg = P.PolicyGradient(root, f.policy, f.fit, T, gamma=0.97, lam=0.9, clip=0.2, ent_coef=0.01, epochs=2, minibatches=2, substeps=1)
        f.policy.set_rng(3, 0)
        torch.cuda.synchronize()
        bufs = pg.buffers()
        for it in range(2):
            seen, wait = [], root.sync
            root.sync = lambda: (seen.append(BatchedPropagator.debug_counters()), wait())[1]
            c0 = BatchedPropagator.debug_counters()
            log = pg.iterate()
            root.sync = wait
            assert seen and seen[0] == c0                   # up to the one wait behind the loop: no copy, no synchronisation
            assert log.shape == (4, 8) and np.isfinite(log).all()
            assert (log[:, 7] == 4 * n).all()               # count: every env of every row of a minibatch
            # the first minibatch of the first epoch runs the parameters the rollout ran: row t of the observation buffer is what
            # the action, the log-probability and the value of step t were formed from
            assert _same(np.float64(log[0, 0]), np.float64(0.0)) and log[0, 2] == 0, (it, log[0])
            assert (log[1:, 0] != 0).all(), (it, log[:, 0])
            assert (log[:, 1] > 0).all() and (log[:, 4] > 0).all() and (log[:, 5] > 0).all()
            hist = {k: _download(bufs[k], dt, cnt) for k, dt, cnt in (("reward", np.float64, T * n), ("reason", np.uint8, T * n), ("value", np.float32, T * n),
                                                                      ("last_value", np.float32, n), ("adv", np.float32, T * n), ("ret", np.float64, T * n))}
            want_adv, want_ret = P.gae_ref(hist["reward"].reshape(T, n), hist["reason"].reshape(T, n), hist["value"].reshape(T, n),
                                           hist["last_value"], 0.97, 0.9)
            assert _same(hist["adv"].reshape(T, n), want_adv) and _same(hist["ret"].reshape(T, n), want_ret)
            ended = hist["reason"].reshape(T, n) != 0
            assert ended.any(axis=1).sum() >= 3 and 0 < ended.sum() < T * n // 2
            # the rollout's last observation row is what the handle holds, and row 0 what it held before
            obs_rows = _download(bufs["obs"], np.float64, (T + 1) * 5 * n).reshape(T + 1, 5, n)
            assert np.array_equal(obs_rows[T], root.get_obs()[0])
        st = f.fit.state()
        assert st["steps"] == 8 and not np.array_equal(st["theta"][10:], params[10:].astype(np.float64))
        assert _same(st["theta"][:10], params[:10].astype(np.float64))
        pg.close()
        f.close()
        root.close()
