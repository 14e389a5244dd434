"""CPU: the numpy restatements of policy-gradient training (basilisk_env_amd/policy_ref.py: gae_ref, fit_pg_dlogits_ref,
fit_pg_dlogits32_ref, fit_pg_loss_ref, fit_pg_stats_ref) - what tests/test_gpu_pg.py holds bsk_gae and bsk_fit_accumulate_pg to -
checked against the textbook sums, against finite differences and against the supervised restatement they must reduce to, and the
argument rules of the bindings, with no device."""
import types

import numpy as np
import pytest

from _device_bits import same as _same
from _fit_bounds import teacher_labels
from _pg_bounds import LEARNING_PG, bandit_step_ref, fd_reach, greedy_agreement, pg_fd_truncation_bound
from _policy_bounds import mlp_bound, observation_like, seeded_policy
from basilisk_env_amd import policy as P
from basilisk_env_amd._lib import FLAG_AUTO_RESET
from basilisk_env_amd.policy_ref import _fit_forward, _fit_inputs, _fit_nets

H = 2.0 ** -13          # the finite-difference step (tests/test_fit_host.py's)


def gae_case(T, N, seed=0):
    """reward, reason, value, last_value for T steps of N envs: terminations at random, and - where there are that many columns and
    rows - one at the first step (column 0), one at the last (column 1), a column terminated everywhere (2) and one with none (3)"""
    rng = np.random.default_rng(500 + seed)
    reward = rng.normal(size=(T, N))
    value = rng.normal(size=(T, N)).astype(np.float32)
    reason = np.where(rng.uniform(size=(T, N)) < 0.2, rng.integers(1, 16, (T, N)), 0).astype(np.uint8)
    if N > 0:
        reason[:, 0] = 0
        reason[0, 0] = 1
    if N > 1:
        reason[:, 1] = 0
        reason[T - 1, 1] = 2
    if N > 2:
        reason[:, 2] = 4
    if N > 3:
        reason[:, 3] = 0
    return reward, reason, value, rng.normal(size=N).astype(np.float32)


@pytest.mark.parametrize("with_last", [False, True])
def test_gae_ref_equals_the_textbook_sum(with_last):
    """adv_t = sum_k (gamma lambda)**k delta_{t+k} over the steps up to and including the first termination at or after t,
    delta_t = r_t + gamma V_{t+1} [reason_t == 0] - V_t, V_T = last_value: the double sum, term by term in Python floats."""
    T, N, g, lam = 7, 5, 0.97, 0.9
    reward, reason, value, last = gae_case(T, N)
    adv, ret = P.gae_ref(reward, reason, value, last if with_last else None, g, lam)
    assert adv.dtype == np.float32 and ret.dtype == np.float64 and adv.shape == ret.shape == (T, N)
    assert reason[0, 0] and reason[T - 1, 1] and reason[:, 2].all() and not reason[:, 3].any()
    v = np.concatenate([value.astype(np.float64), (last.astype(np.float64) if with_last else np.zeros(N))[None, :]])
    for j in range(N):
        for t in range(T):
            want, w = 0.0, 1.0
            for k in range(t, T):
                run = reason[k, j] == 0
                want += w * (reward[k, j] + (g * v[k + 1, j] if run else 0.0) - v[k, j])
                if not run:
                    break
                w *= g * lam
            scale = max(1.0, abs(want))
            assert abs(float(ret[t, j]) - (want + v[t, j])) <= 1e-12 * scale, (t, j)
            assert adv[t, j] == np.float32(ret[t, j] - v[t, j]) or abs(float(adv[t, j]) - want) <= 2.0 ** -23 * scale, (t, j)
    # a terminated step's advantage is its own delta, whatever follows
    assert _same(adv[:, 2], (reward[:, 2] - value[:, 2].astype(np.float64)).astype(np.float32))


def _relu_pattern(spec, theta, obs):
    scale, shift, a, _ = _fit_nets(spec, theta, True)
    x, n = _fit_inputs(scale, shift, obs, True)
    return [h[:, :n] > 0 for h in _fit_forward(a, spec.activation, x, True)[1:-1]] if spec.activation == "relu" else []


def _fd_inputs(spec, theta, obs, ppo):
    """actions, advantages of both signs and zero, alive bytes, and - PPO - old log-probabilities a fixed distance from the fp64
    log-probabilities of the actions: ratios exp(+-0.05) inside the clip range and exp(+-0.5) beyond either edge, each met with
    advantages of both signs"""
    n = obs.shape[1]
    rng = np.random.default_rng(8)
    actions = rng.integers(0, 3, n)
    adv = rng.normal(size=n).astype(np.float32)
    adv[[3, 17]] = 0.0
    alive = np.ones(n, np.uint8)
    alive[7] = 0
    if not ppo:
        return actions, adv, alive, None
    scale, shift, a, _ = _fit_nets(spec, theta, True)
    x, _ = _fit_inputs(scale, shift, obs, True)
    l = _fit_forward(a, spec.activation, x, True)[-1][:, :n]
    z = l - l.max(axis=0)
    lpa = (z - np.log(np.exp(z).sum(axis=0)))[actions, np.arange(n)]
    shift_by = np.tile([0.05, -0.05, 0.5, -0.5], n // 4 + 1)[:n]
    return actions, adv, alive, (lpa - shift_by).astype(np.float32)


@pytest.mark.parametrize("ent_coef", [0.0, 0.05])
@pytest.mark.parametrize("ppo", [False, True])
@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_the_fp64_pg_gradient_equals_central_finite_differences(act, ppo, ent_coef):
    """d loss / d theta_p from fit_pg_dlogits_ref(fp64=True) + fit_backward_ref(fp64=True) against the central difference of
    fit_pg_loss_ref, for every parameter p >= 10 of a (16,) network on 40 samples.  The tolerance is derived (tests/_pg_bounds.py):
      truncation  h**2 / 6 * the summed bound on the third derivative of each sample's loss along theta_p;
      rounding    as tests/test_fit_host.py argues: fp64 logits carry at most 2 * 2**-29 e_l; lp_a moves by at most twice the
                  largest logit error, the surrogate -A r by |A| r times that, the entropy (slope sum_i |p_i (lp_i + H)| <= 2 log 3)
                  by 2 log 3 times it, plus 32 roundings of 2**-53 on each term's magnitude; two losses, divided by 2 h.
    No sample's ratio may cross a clip edge along a segment (the loss has a kink there): asserted.  relu: a parameter whose
    perturbation switches a hidden unit is left out, and counted."""
    clip, n = 0.2, 40
    spec, params = seeded_policy((16,), act, seed=2)
    theta = params.astype(np.float64)
    obs = observation_like(n, 5)
    actions, adv, alive, old = _fd_inputs(spec, theta, obs, ppo)
    on = alive != 0
    args = (spec, theta, obs, actions, adv, old, clip, ent_coef, alive)
    g = P.fit_pg_dlogits_ref(*args, fp64=True)
    grad = P.fit_backward_ref(spec, theta, obs, g, None, fp64=True).sum(axis=0)
    assert not g[:, ~on].any() and not grad[:10].any()

    l64, e_l, _, _ = mlp_bound(spec, params, obs)
    t = P.fit_pg_terms_ref(l64, actions, adv, old, clip, ent_coef, on, fp64=True)
    trunc, reach = pg_fd_truncation_bound(spec, params, obs, on, H, adv, t["r"] if ppo else None, t["clipped"], ent_coef)
    if ppo:
        lo, hi = P.pg_clip_edges(clip)
        assert not fd_reach(t["r"], reach, clip).any()
        A = adv.astype(np.float64)
        # both edges are crossed, by advantages of the sign that clips and of the sign that does not; some advantage is zero
        assert ((t["r"] > hi) & (A > 0)).sum() >= 2 and ((t["r"] > hi) & (A < 0)).sum() >= 2
        assert ((t["r"] < lo) & (A < 0)).sum() >= 2 and ((t["r"] < lo) & (A > 0)).sum() >= 2
        assert 4 <= t["clipped"].sum() < n // 2
    assert (adv == 0).sum() == 2 and (adv > 0).any() and (adv < 0).any()
    e_logit = 2.0 * 2.0 ** -29 * e_l.max(axis=0)
    A, r = np.abs(adv.astype(np.float64)), t["r"]
    lpa = np.abs(t["d"] + (0.0 if old is None else old.astype(np.float64)))
    if not ppo:
        z = l64 - l64.max(axis=0)
        lpa = np.abs((z - np.log(np.exp(z).sum(axis=0)))[actions, np.arange(n)])
    ec = float(np.float32(ent_coef))
    e_term = (A * r * np.expm1(2.0 * e_logit) if ppo else A * 2.0 * e_logit) + ec * 2.0 * np.log(3.0) * e_logit
    e_term = e_term + 32 * 2.0 ** -53 * (A * r + A * lpa + ec * np.log(3.0) + np.abs(l64).max(axis=0))
    rounding = 2.0 * e_term[on].sum() / (2.0 * H)

    base = _relu_pattern(spec, theta, obs)
    worst, skipped = 0.0, 0
    loss = lambda th: P.fit_pg_loss_ref(spec, th, obs, actions, adv, old, clip, ent_coef, alive)      # noqa: E731
    for p in range(10, theta.size):
        up, dn = theta.copy(), theta.copy()
        up[p] += H
        dn[p] -= H
        if any(not (np.array_equal(a, b) and np.array_equal(a, c)) for a, b, c in zip(base, _relu_pattern(spec, up, obs), _relu_pattern(spec, dn, obs))):
            skipped += 1
            continue
        fd = (loss(up) - loss(dn)) / (up[p] - dn[p])
        tol = trunc[p] + rounding
        worst = max(worst, abs(fd - grad[p]) / tol)
        assert abs(fd - grad[p]) <= tol, (p, fd, grad[p], tol)
    print("%s ppo=%s ent=%g: %d parameters, %d across a kink, worst error / tolerance %.3g, tolerance up to %.3g on gradients up to %.3g"
          % (act, ppo, ent_coef, theta.size - 10, skipped, worst, (trunc + rounding).max(), np.abs(grad).max()))
    assert skipped <= (theta.size - 10) // 8 and np.abs(grad[10:]).max() > 100 * (trunc[10:] + rounding).max()


@pytest.mark.parametrize("net", [((16,), "relu"), ((80, 48), "relu"), ((32,), "tanh")])
def test_unit_advantages_without_a_ratio_are_the_supervised_deltas_bit_for_bit(net):
    spec, params = seeded_policy(*net, seed=3)
    n = 200
    obs = observation_like(n, 1)
    rng = np.random.default_rng(301)
    actions = rng.integers(0, 3, n).astype(np.int32)
    actions[[2, n - 3]] = [3, -1]
    alive = np.ones(n, np.uint8)
    alive[[5, n // 2]] = 0
    want, _ = P.fit_dlogits32_ref(spec, params, obs, actions, alive)
    got = P.fit_pg_dlogits32_ref(spec, params, obs, actions, np.ones(n, np.float32), None, 0.2, 0.0, alive)
    assert got.dtype == np.float32 and _same(got, want) and np.count_nonzero(got) == 3 * (n - 4)
    assert _same(P.fit_pg_dlogits_ref(spec, params, obs, actions, np.ones(n, np.float32), alive=alive, fp64=False), want)
    # the row beside it: no ratio, so no KL and nothing clipped; the surrogate column counts the unit advantages
    row = P.fit_pg_stats_ref(spec, params, obs, actions, np.ones(n, np.float32), None, 0.2, alive)
    assert row[0] == 0.0 and row[2] == 0.0 and row[3] == n - 4 and 0.0 < row[1] < (n - 4) * np.log(3.0)


def test_zero_advantages_and_own_log_probabilities():
    """A == 0 with ec == 0: +0.0 deltas, bit for bit, in either mode.  Old log-probabilities that are ``act_ref``'s own: d is +0.0
    for every sample, so the ratio is 1, nothing is clipped, the KL column is +0.0 and the surrogate column is the sum of A."""
    spec, params = seeded_policy((16,), "relu", seed=4)
    n = 130
    obs = observation_like(n, 2)
    l = P.mlp_ref(spec, params, obs)[0]
    actions, logp = P.act_ref(l, "sample", seed=5, draw=2)
    adv = np.random.default_rng(9).normal(size=n).astype(np.float32)
    adv[::3] = 0.0
    for old in (None, logp):
        g = P.fit_pg_dlogits32_ref(spec, params, obs, actions, adv, old, 0.2, 0.0)
        assert _same(g[:, ::3], np.zeros((3, len(adv[::3])), np.float32)) and g[:, 1::3].all()
    t = P.fit_pg_terms_ref(l, actions, adv, logp)
    assert _same(t["d"], np.zeros(n, np.float32)) and _same(t["r"], np.ones(n, np.float32)) and not t["clipped"].any()
    row = P.fit_pg_stats_ref(spec, params, obs, actions, adv, logp, 0.2)
    want = 0.0
    blocks = [adv[b:b + 64].astype(np.float64) for b in range(0, n, 64)]
    for part in [sum(b.tolist(), 0.0) for b in blocks]:
        want = want + part
    assert _same(np.float64(row[0]), np.float64(0.0)) and row[2] == 0.0 and _same(np.float64(row[3]), np.float64(want))
    # with an entropy bonus a zero advantage still has the bonus's gradient
    g = P.fit_pg_dlogits32_ref(spec, params, obs, actions, adv, logp, 0.2, 0.01)
    assert g[:, ::3].any()


def test_argument_rules_need_no_device():
    assert P.PG_STATS_COLUMNS == ("kl_sum", "entropy_sum", "clipped", "surrogate_sum")
    assert P.check_pg(0.2, 0.01) == (0.2, 0.01) and P.check_pg(7.0, 0.0, with_logp_old=False) == (7.0, 0.0)
    for clip in (0.0, 1.0, -0.1, 1.5, np.nan, np.inf):
        with pytest.raises(ValueError):
            P.check_pg(clip, 0.0)
    for ent in (-1e-9, np.nan, np.inf):
        with pytest.raises(ValueError):
            P.check_pg(0.2, ent)
        with pytest.raises(ValueError):
            P.check_pg(0.2, ent, with_logp_old=False)
    assert P.check_gae(3, 5, 5, 1.0, 0.0) == (3, 5, 5, 1.0, 0.0)
    for bad in ((0, 5, 5, 0.9, 0.9), (3, 0, 5, 0.9, 0.9), (3, 5, 4, 0.9, 0.9), (3, 5, 5, 1.01, 0.9), (3, 5, 5, 0.9, -0.1),
                (3, 5, 5, np.nan, 0.9), (3, 5, 5, 0.9, np.inf), (3.0, 5, 5, 0.9, 0.9)):
        with pytest.raises(ValueError):
            P.check_gae(*bad)
    # the loop: its own numbers first, then the env, the policy and the fit - none of which is touched before it refuses
    good = dict(n_steps=8, gamma=0.99, lam=0.95, clip=0.2, ent_coef=0.01, epochs=2, minibatches=2, substeps=1)
    assert P.check_pg_loop(**good) == (8, 0.99, 0.95, 0.2, 0.01, 2, 2, 1)
    for key, value in (("n_steps", 0), ("n_steps", 7), ("epochs", 0), ("minibatches", 3), ("substeps", 0), ("gamma", 1.5), ("lam", -1.0),
                       ("clip", 1.0), ("ent_coef", -0.5), ("epochs", 1.5)):
        with pytest.raises(ValueError):
            P.check_pg_loop(**dict(good, **{key: value}))
    with_value, without = P.check_spec((16,), "relu", (16,)), P.check_spec((16,), "relu")
    cfg = lambda flags: types.SimpleNamespace(flags=flags)                                   # noqa: E731
    env = lambda flags, device=0: types.SimpleNamespace(cfg=cfg(flags), device=device, n_envs=64)          # noqa: E731
    pol = types.SimpleNamespace(spec=with_value, device=0)
    fit = types.SimpleNamespace(policy=pol)
    for e, p, f, word in ((env(0), pol, fit, "AUTO_RESET"), (env(FLAG_AUTO_RESET), types.SimpleNamespace(spec=without, device=0), fit, "value network"),
                          (env(FLAG_AUTO_RESET), pol, types.SimpleNamespace(policy=None), "another policy"),
                          (env(FLAG_AUTO_RESET, device=1), pol, fit, "device")):
        with pytest.raises(ValueError) as err:
            P.PolicyGradient(e, p, f, 8)
        assert word in str(err.value)
    with pytest.raises(ValueError):
        P.PolicyGradient(env(FLAG_AUTO_RESET), pol, fit, 8, minibatches=3)


def test_the_reference_alone_learns_the_bandit():
    """The learning recipe (``_pg_bounds.LEARNING_PG``) on the numpy restatement alone, sampling seeds 0 .. 4: the recorded greedy
    agreement with the teacher at the start, and the recorded lowest one after the steps - which clears the initial one by more
    than half the batch.  tests/test_gpu_pg.py asks the device for the midpoint of the two."""
    L = LEARNING_PG
    spec, params = seeded_policy(L["hidden"], "relu", seed=L["seed"])
    obs = observation_like(256)
    teacher = teacher_labels(obs)
    assert greedy_agreement(spec, params, obs, teacher) == L["initial"]
    finals = []
    for seed in range(5):
        state = (params.astype(np.float64), np.zeros(params.size), np.zeros(params.size), np.ones(2), 0)
        for k in range(L["steps"]):
            state = bandit_step_ref(spec, state, obs, teacher, seed, k, L["lr"])
        finals.append(greedy_agreement(spec, state[0], obs, teacher))
    print("greedy agreement with the teacher: %d of 256 -> %r" % (L["initial"], finals))
    assert min(finals) == L["final_min"] and L["final_min"] - L["initial"] > 128
