"""CPU: the numpy restatements of the policy fit (basilisk_env_amd/policy_ref.py: fit_dlogits_ref, fit_backward_ref,
fit_accumulate_ref, fit_step_ref, fit_loss_ref) - what tests/test_gpu_fit.py holds the kernels of csrc/bsk_fit.hip to - checked
against finite differences and against their own definition's corner cases, and the argument rules of the binding, with no device."""
import types

import numpy as np
import pytest

from _fit_bounds import LEARNING, fd_truncation_bound, teacher_labels
from _policy_bounds import mlp_bound, observation_like, seeded_policy
from basilisk_env_amd import policy as P
from basilisk_env_amd import planning
from basilisk_env_amd.policy_ref import _adam_step_ref, _fit_forward, _fit_inputs, _fit_nets

H = 2.0 ** -13          # the finite-difference step


def _relu_pattern(spec, theta, obs):
    """which hidden units of both networks are on, per sample: the linear region theta lies in"""
    scale, shift, a, v = _fit_nets(spec, theta, True)
    x, n = _fit_inputs(scale, shift, obs, True)
    on = []
    for layers, act in ((a, spec.activation), (v, spec.value_activation)):
        if layers is not None and act == "relu":
            on += [h[:, :n] > 0 for h in _fit_forward(layers, act, x, True)[1:-1]]
    return on


@pytest.mark.parametrize("hidden,act,vh", [((16,), "relu", None), ((32, 16), "tanh", None), ((16,), "relu", (16,))])
def test_the_fp64_gradient_equals_central_finite_differences(hidden, act, vh):
    """d loss / d theta_p from fit_dlogits_ref + fit_backward_ref(fp64=True) against (L(theta + h e_p) - L(theta - h e_p)) / (2 h)
    of fit_loss_ref, for EVERY parameter p >= 10, h = 2**-13 (the divisor is the difference of the two perturbed floats, exactly).
    The tolerance is derived, not tuned (tests/_fit_bounds.py):
      truncation  h**2 / 6 * the sum over the samples of the bound on the third derivative of the sample's loss along theta_p;
      rounding    the loss is a sum of 20 terms each computed in fp64 from logits that carry at most e_l * 2**-29 (``mlp_bound``'s
                  f32 bound scaled by the ratio of the unit roundoffs, as _policy_bounds' FP64_SLACK argues; doubled, because the bound
                  is formed at theta and used at theta +- h) - logsumexp and l_label are 1-Lipschitz in the largest logit error, the
                  squared value error has the slope c |v - T| - plus 16 roundings of 2**-53 on each term's own magnitude; the two
                  losses' errors add and are divided by 2 h.
    relu is differentiable only inside a linear region: a parameter whose +-h perturbation switches a hidden unit of some sample is
    left out of the comparison (finite differences say nothing across a kink); they are few, and counted."""
    spec, params = seeded_policy(hidden, act, vh, seed=2)
    theta = params.astype(np.float64)
    obs = observation_like(20, 5)
    rng = np.random.default_rng(6)
    labels = rng.integers(0, 3, 20)
    alive = np.ones(20, np.uint8)
    alive[7] = 0
    targets, vc = (rng.normal(size=20), 0.5) if vh else (None, 0.0)
    g, gv = P.fit_dlogits_ref(spec, theta, obs, labels, alive, targets, vc)
    G = P.fit_backward_ref(spec, theta, obs, g, gv, fp64=True)
    assert G.shape == (1, theta.size) and not G[:, :10].any()
    grad = G.sum(axis=0)
    on = alive != 0
    trunc = fd_truncation_bound(spec, params, obs, on, H, targets, vc)
    l64, e_l, v64, e_v = mlp_bound(spec, params, obs)
    d = l64 - l64.max(axis=0)
    ce = np.log(np.exp(d).sum(axis=0)) - d[labels, np.arange(20)]
    e_term = 2.0 * 2.0 ** -29 * 2.0 * e_l.max(axis=0) + 16 * 2.0 ** -53 * (np.abs(ce) + np.abs(l64).max(axis=0))
    if vh:
        dv = np.abs(v64 - targets)
        e_term = e_term + vc * (dv * 2.0 * 2.0 ** -29 * e_v + 16 * 2.0 ** -53 * dv * dv)
    rounding = 2.0 * e_term[on].sum() / (2.0 * H)
    base = _relu_pattern(spec, theta, obs)
    worst, skipped = 0.0, 0
    for p in range(10, theta.size):
        up, dn = theta.copy(), theta.copy()
        up[p] += H
        dn[p] -= H
        if any(not (np.array_equal(a, b) and np.array_equal(a, c)) for a, b, c in zip(base, _relu_pattern(spec, up, obs), _relu_pattern(spec, dn, obs))):
            skipped += 1
            continue
        fd = (P.fit_loss_ref(spec, up, obs, labels, alive, targets, vc) - P.fit_loss_ref(spec, dn, obs, labels, alive, targets, vc)) / (up[p] - dn[p])
        tol = trunc[p] + rounding
        worst = max(worst, abs(fd - grad[p]) / tol)
        assert abs(fd - grad[p]) <= tol, (p, fd, grad[p], tol)
    print("%r %s: %d parameters, %d across a kink, worst error / tolerance %.3g, tolerance up to %.3g on gradients up to %.3g"
          % (hidden, act, theta.size - 10, skipped, worst, (trunc + rounding).max(), np.abs(grad).max()))
    assert skipped <= (theta.size - 10) // 8 and np.abs(grad[10:]).max() > 100 * (trunc[10:] + rounding).max()
    # the value network gets its gradient with targets only
    a_end = 10 + sum(o * i + o for o, i in P.layer_shapes(spec)[0])
    assert (np.abs(grad[a_end:]).max() > 0) if vh else a_end == theta.size


def test_masked_samples_and_the_tail_contribute_exact_zeros():
    spec, params = seeded_policy((32, 16), "relu", (16,), seed=3)
    obs = observation_like(70, 1)
    rng = np.random.default_rng(8)
    labels = rng.integers(0, 3, 70).astype(np.int32)
    targets = rng.normal(size=70)
    alive = np.ones(70, np.uint8)
    masked = np.array([3, 17, 40, 63, 64, 69])
    alive[masked[:3]] = 0
    labels[masked[3:]] = [3, -1, 7]
    g, gv = P.fit_dlogits32_ref(spec, params, obs, labels, alive, targets, 0.5)
    assert not g[:, masked].any() and not gv[masked].any() and not np.signbit(g[:, masked]).any()
    g64, gv64 = P.fit_dlogits_ref(spec, params, obs, labels, alive, targets, 0.5)
    assert not g64[:, masked].any() and not gv64[masked].any()
    G = P.fit_backward_ref(spec, params, obs, g, gv)
    assert G.shape == (2, params.size) and G.dtype == np.float32
    # the 64 unmasked samples alone, each in the block it was in: the same bits
    keep = np.setdiff1d(np.arange(70), masked)
    alone = np.zeros((2, params.size), np.float32)
    for b, idx in enumerate((keep[keep < 64], keep[keep >= 64])):
        # (a block's chains walk its samples in ascending order, and a masked sample adds +0.0 * h = +0.0: leaving it out changes nothing)
        alone[b] = P.fit_backward_ref(spec, params, obs[:, idx], g[:, idx], gv[idx])[0]
    assert np.array_equal(G.view(np.int32), alone.view(np.int32))
    assert np.array_equal(G.view(np.int32), P.fit_backward_ref(spec, params, obs, g, gv).view(np.int32))
    # the count leaves the masked samples out, and so do the diagnostics
    row = P.fit_stats_ref(spec, params, obs, labels, alive, targets)
    assert row[3] == 64 and 0 <= row[2] <= 64 and row[0] > 0 and row[1] > 0
    A, count = P.fit_accumulate_ref(np.zeros(params.size), 0, G, row[3])
    A2, count2 = P.fit_accumulate_ref(A, count, G, row[3])
    assert count == 64 and count2 == 128 and np.array_equal(A, G[0].astype(np.float64) + G[1].astype(np.float64))
    assert np.array_equal(A2, (A + G[0].astype(np.float64)) + G[1].astype(np.float64))
    # without value deltas the value network's columns are zero
    a_end = 10 + sum(o * i + o for o, i in P.layer_shapes(spec)[0])
    Ga = P.fit_backward_ref(spec, params, obs, g)
    assert not Ga[:, a_end:].any() and np.array_equal(Ga[:, :a_end], G[:, :a_end]) and G[:, a_end:].any()


def test_a_step_with_no_sample_moves_nothing_and_a_step_descends():
    rng = np.random.default_rng(9)
    n = 40
    theta, m, v, A = rng.normal(size=n), rng.normal(size=n), rng.uniform(size=n), rng.normal(size=n)
    bp = np.array([0.81, 0.998])
    out = P.fit_step_ref(theta, m, v, bp, 5, A, 0, 1e-2, 0.9, 0.999, 1e-8, 1e-3)
    for got, want in zip(out[:4], (theta, m, v, bp)):
        assert np.array_equal(got, want)
    assert out[4] == 5 and not out[5].any() and out[6] == 0
    out = P.fit_step_ref(theta, np.zeros(n), np.zeros(n), np.ones(2), 0, A, 8, 1e-2, 0.9, 0.999, 1e-8, 0.0, n_update=30)
    assert np.array_equal(out[0][:10], theta[:10]) and np.array_equal(out[0][30:], theta[30:]) and not out[1][30:].any()
    # the first Adam step is lr * sign(g) up to eps: against the gradient
    assert np.allclose(out[0][10:30], theta[10:30] - 1e-2 * np.sign(A[10:30]), rtol=0, atol=1e-8)
    assert np.array_equal(out[3], np.array([0.9, 0.999])) and out[4] == 1 and not out[5].any() and out[6] == 0
    # ... and it is the evolution strategy's update with the other sign: one text behind both
    g = A[10:] / np.float64(8)
    m2, v2, step, bp2 = _adam_step_ref(np.zeros(n - 10), np.zeros(n - 10), np.ones(2), g, np.float64(1e-2), np.float64(0.9),
                                                    np.float64(0.999), np.float64(1e-8))
    full = P.fit_step_ref(theta, np.zeros(n), np.zeros(n), np.ones(2), 0, A, 8, 1e-2, 0.9, 0.999, 1e-8, 0.0)
    assert np.array_equal(full[0][10:], theta[10:] - step) and np.array_equal(full[1][10:], m2) and np.array_equal(full[2][10:], v2)


class _Fake(object):
    def __init__(self, shape, typestr, strides=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (0x7000, False), "version": 2, "strides": strides}


def test_argument_rules_need_no_device():
    nan, inf = float("nan"), float("inf")
    good = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0.5)
    assert P.check_fit(*good) == good and P.check_fit(0, 0, 0, 1, 0, 0) == (0.0, 0.0, 0.0, 1.0, 0.0, 0.0)
    for k, bad in ((0, (-1e-3, nan, inf)), (1, (-0.1, 1.0, nan)), (2, (1.0, 1.5, nan)), (3, (0.0, -1.0, nan, inf)), (4, (-1e-3, nan, inf)),
                   (5, (-0.5, nan, inf))):
        for x in bad:
            args = list(good)
            args[k] = x
            with pytest.raises(ValueError):
                P.check_fit(*args)
            with pytest.raises(ValueError):                  # the binding refuses before it touches the library or the policy
                P.PolicyFit(None, *args)
    spec = P.check_spec((16,), "relu")
    spec_v = P.check_spec((16,), "relu", (16,))
    assert P.check_fit_batch(spec, 5, 5, None, 5) == 5 and P.check_fit_batch(spec_v, 1, 1, 1, None) == 1
    for args in ((spec, 0), (spec, -3), (spec, 2.5), (spec, True), (spec, 5, 4), (spec, 5, 5, 5), (spec_v, 5, 5, 4), (spec, 5, 5, None, 6)):
        with pytest.raises(ValueError):
            P.check_fit_batch(*args)
    # accumulate's own checks come before the handle is asked for: a closed object with a policy's spec is enough
    fit = P.PolicyFit.__new__(P.PolicyFit)
    fit.policy, fit._p = types.SimpleNamespace(spec=spec), None
    obs, labels = _Fake((5, 8), "<f8"), _Fake((8,), "<i4")
    for args in ((_Fake((5, 8), "<f4"), labels), (_Fake((4, 8), "<f8"), labels), (_Fake((5, 8), "<f8", (72, 16)), labels), (0x7000, labels),
                 (obs, _Fake((8,), "<i8")), (obs, _Fake((7,), "<i4")), (obs, None), (obs, labels, _Fake((8,), "<f8")),
                 (obs, labels, None, _Fake((9,), "|u1")), (obs, labels, None, None, _Fake((8, 3), "<f4")), (obs, labels, 0x8000)):
        with pytest.raises(ValueError):
            fit.accumulate(*args)
    with pytest.raises(RuntimeError, match="policy fit is closed"):
        fit.accumulate(obs, labels)
    for args in ((0, "expert"), (2.0, "expert"), (True, "policy"), (3, "dagger")):
        with pytest.raises(ValueError):
            planning.check_distill_args(*args)
    assert planning.check_distill_args(4, "policy") == 4
    assert "PolicyFit" in dir(P) and P.FIT_STATS_COLUMNS == ("nll_sum", "value_loss_sum", "correct", "count")


def test_the_reference_alone_learns_the_teacher_rule():
    """The learning check's set-up, held to the reference alone: relu (32,), seed 0, 60 rounds of one accumulate of all 256 samples
    and one step, lr = 1e-2, Adam's defaults - the first values tried.  The final mean cross-entropy is below a QUARTER of the
    initial one here; tests/test_gpu_fit.py then asks the device for below half."""
    spec, params = seeded_policy(LEARNING["hidden"], "relu", seed=LEARNING["seed"])
    obs = observation_like(256)
    labels = teacher_labels(obs)
    assert min(np.bincount(labels, minlength=3)) >= 20            # (every action is somebody's label)
    state = (params.astype(np.float64), np.zeros(params.size), np.zeros(params.size), np.ones(2), 0)
    rows = []
    for _ in range(LEARNING["steps"] + 1):
        now = state[0].astype(np.float32)
        rows.append(P.fit_stats_ref(spec, now, obs, labels))
        g, _ = P.fit_dlogits32_ref(spec, now, obs, labels)
        A, count = P.fit_accumulate_ref(np.zeros(params.size), 0, P.fit_backward_ref(spec, now, obs, g), rows[-1][3])
        state = P.fit_step_ref(*state, A, count, LEARNING["lr"], 0.9, 0.999, 1e-8, 0.0)[:5]
    first, last = rows[0], rows[-1]
    print("mean cross-entropy %.4f -> %.4f, correct %d -> %d of 256" % (first[0] / 256, last[0] / 256, first[2], last[2]))
    assert first[3] == last[3] == 256 and last[0] < 0.25 * first[0] and last[2] >= first[2]
