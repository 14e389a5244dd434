"""CPU: the numpy restatements of what conditions the policy-gradient update as PPO2 does (basilisk_env_amd/policy_ref.py:
adv_normalize_ref, fit_grad_norm_ref, fit_step_ref's max_grad_norm) - what tests/test_gpu_pg_cond.py holds bsk_adv_normalize and the
clipped bsk_fit_step to - checked against numpy.mean / numpy.std / numpy.linalg.norm in plain f64 within the bounds of
tests/_pg_cond_bounds.py, and the argument rules of the bindings, with no device."""
import numpy as np
import pytest

from _device_bits import same as _same
from _pg_cond_bounds import adv_case, adv_moments_bound, adv_out_bound, clipped_norm_rel_bound, grad_norm_rel_bound
from basilisk_env_amd import _lib
from basilisk_env_amd import policy as P


# ------------------------------------------------------------------------------------------------------------------ advantages
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e4])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("rows,n", [(1, 1), (1, 63), (2, 64), (7, 65), (2, 300), (3, 4097), (1030, 3), (1030, 70)])
def test_adv_normalize_ref_is_numpys_mean_and_std_within_the_derived_bound(rows, n, masked, scale):
    eps = 1e-8
    adv, alive = adv_case(rows, n, rows * 10 + n, scale, masked and rows * n > 8)
    out, mom = P.adv_normalize_ref(adv, alive, eps)
    assert out.dtype == np.float32 and out.shape == adv.shape and mom.dtype == np.float64 and mom.shape == (4,)
    on = np.ones(adv.shape, bool) if alive is None else alive != 0
    x = adv.astype(np.float64)[on]
    N, M = x.size, float(np.abs(x).max())
    mean, sd = np.mean(x), np.std(x)
    E_mean, E_sd = adv_moments_bound(N, M, sd)
    print("rows %d n %d scale %g: N %d, |mean - numpy| %.3e (bound %.3e), |sd - numpy| %.3e (bound %.3e)"
          % (rows, n, scale, N, abs(mom[0] - mean), E_mean, abs(mom[1] - sd), E_sd))
    assert mom[3] == N and abs(mom[0] - mean) <= E_mean and abs(mom[1] - sd) <= E_sd
    assert _same(mom[2], np.float64(1.0) / (mom[1] + np.float64(eps)))
    want = (x - mean) / (sd + eps)
    err = np.abs(out[on].astype(np.float64) - want)
    bound = adv_out_bound(x, mean, sd, mom[1], eps, E_mean, E_sd)
    print("    max |out - numpy| %.3e, max bound %.3e, max ratio %.3f" % (err.max(), bound.max(), (err / bound).max()))
    assert (err <= bound).all()
    assert _same(out[~on], np.zeros(int((~on).sum()), np.float32))               # +0.0f, bit for bit
    if N > 100:
        # what the normalisation is for: mean 0 and standard deviation sd / (sd + eps), each to the rounding of the outputs to f32 -
        # 2**-24 |out| per sample, whose root mean square is at most 1 - and the bound above, twice over for slack
        o = out[on].astype(np.float64)
        assert abs(o.mean()) <= 2.0 ** -23 + 2.0 * bound.max() and abs(o.std() - sd / (sd + eps)) <= 2.0 ** -23 + 2.0 * bound.max()


def test_adv_normalize_ref_degenerate_cases():
    adv, _ = adv_case(3, 70, 1)
    # nothing counts: the moments are four +0.0 and nothing is written
    out, mom = P.adv_normalize_ref(adv, np.zeros(adv.shape, np.uint8))
    assert _same(out, adv) and _same(mom, np.zeros(4))
    # one sample: mean = x, var = x * x / 1 - x * x = 0 exactly, the sample becomes (x - x) * inv = +0.0
    alive = np.zeros(adv.shape, np.uint8)
    alive[1, 65] = 1
    out, mom = P.adv_normalize_ref(adv, alive, 1e-8)
    x = np.float64(adv[1, 65])
    assert x != 0 and _same(mom, np.array([x, 0.0, np.float64(1.0) / np.float64(1e-8), 1.0]))
    assert _same(out, np.zeros(adv.shape, np.float32))
    # all samples equal (a power of two times the count: every sum is exact): sd = 0 and every output +0.0
    out, mom = P.adv_normalize_ref(np.full((4, 64), 0.75, np.float32), None, 1e-8)
    assert _same(mom, np.array([0.75, 0.0, 1e8, 256.0])) and _same(out, np.zeros((4, 64), np.float32))
    # ... and in general finite, whatever the rounding of the mean leaves: eps carries the division
    out, mom = P.adv_normalize_ref(np.full((7, 300), 0.1, np.float32), None, 1e-8)
    assert mom[3] == 2100 and mom[1] < 1e-7 and np.isfinite(out).all() and np.abs(out).max() < 1e-6
    # a sample that does not count does not enter, whatever it holds
    adv, alive = adv_case(2, 130, 2, masked=True)
    other = adv.copy()
    other[alive == 0] = np.float32(1e30)
    a, b = P.adv_normalize_ref(adv, alive), P.adv_normalize_ref(other, alive)
    assert _same(a[0], b[0]) and _same(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------------ the clip
def _accumulators(n_params, seed, scale=1.0):
    rng = np.random.default_rng(9100 + seed)
    return rng.normal(0.0, scale, n_params) * rng.uniform(0.0, 3.0, n_params)


@pytest.mark.parametrize("n_params,n_update", [(28, 28), (500, 400), (1034, 1034), (1035, 1035), (20000, 20000), (20000, 17000)])
def test_fit_grad_norm_ref_is_numpys_norm_within_the_derived_bound(n_params, n_update):
    A, count = _accumulators(n_params, n_params), 777
    want = np.linalg.norm(A[10:n_update] / count)
    for max_norm in (want * 0.25, want * 4.0):
        norm, scale = P.fit_grad_norm_ref(A, count, n_update, max_norm)
        rel = grad_norm_rel_bound(n_update - 10)
        print("n %d: |norm - numpy| / norm %.3e, bound %.3e" % (n_update - 10, abs(norm - want) / want, rel))
        assert abs(norm - want) <= rel * want
        assert _same(scale, np.float64(max_norm) / max(norm, np.float64(max_norm)))
        assert (scale == 1.0) == (max_norm > want)
    # the entries the step does not move do not enter
    other = A.copy()
    other[:10], other[n_update:] = 1e30, 1e30
    assert _same(np.array(P.fit_grad_norm_ref(other, count, n_update, 0.5)), np.array(P.fit_grad_norm_ref(A, count, n_update, 0.5)))
    assert P.fit_grad_norm_ref(A, 0, n_update, 0.5) == (0.0, 1.0)
    with pytest.raises(ValueError):
        P.fit_grad_norm_ref(A, count, n_update, 0.0)


def _state(n_params, seed):
    rng = np.random.default_rng(9200 + seed)
    return (rng.normal(size=n_params), rng.normal(0.0, 0.1, n_params), rng.uniform(0.0, 0.1, n_params), np.array([0.9 ** 3, 0.999 ** 3]), 3)


ADAM = (1e-2, 0.9, 0.999, 1e-8, 1e-3)


@pytest.mark.parametrize("n_update", [None, 300])
def test_fit_step_ref_with_a_bound_above_the_norm_is_the_default_bit_for_bit(n_update):
    n_params = 1500
    state, A = _state(n_params, 1), _accumulators(n_params, 1)
    plain = P.fit_step_ref(*state, A, 50, *ADAM, n_update=n_update)
    assert all(_same(np.asarray(a), np.asarray(b)) for a, b in zip(plain, P.fit_step_ref(*state, A, 50, *ADAM, n_update=n_update, max_grad_norm=0.0)))
    norm = P.fit_grad_norm_ref(A, 50, n_update or n_params, 1.0)[0]
    big = P.fit_step_ref(*state, A, 50, *ADAM, n_update=n_update, max_grad_norm=float(norm) * 2.0)
    assert all(_same(np.asarray(a), np.asarray(b)) for a, b in zip(plain, big))
    assert not np.array_equal(plain[0], state[0]) and plain[4] == 4
    # exactly at the norm: norm > max_norm is false, the scale is max_norm / max_norm
    at = P.fit_step_ref(*state, A, 50, *ADAM, n_update=n_update, max_grad_norm=float(norm))
    assert all(_same(np.asarray(a), np.asarray(b)) for a, b in zip(plain, at))
    small = P.fit_step_ref(*state, A, 50, *ADAM, n_update=n_update, max_grad_norm=float(norm) / 2.0)
    assert not np.array_equal(small[1], plain[1]) and small[4] == 4
    # count == 0: nothing moves, with or without
    for kw in ({}, {"max_grad_norm": 0.5}):
        still = P.fit_step_ref(*state, A, 0, *ADAM, n_update=n_update, **kw)
        assert all(_same(np.asarray(a), np.asarray(b)) for a, b in zip(still[:5], state)) and not still[5].any()


@pytest.mark.parametrize("n_params", [28, 1500, 20000])
def test_a_small_bound_brings_the_gradients_norm_to_it(n_params):
    """lr and weight_decay aside, what Adam is fed is (A / count) * scale: read back through the first moment with beta1 = 0"""
    A, count, max_norm = _accumulators(n_params, 2, 100.0), 64, 0.5
    norm, scale = P.fit_grad_norm_ref(A, count, n_params, max_norm)
    assert norm > 4 * max_norm and scale < 0.25          # (the case: the clip bites)
    z = np.zeros(n_params)
    m = P.fit_step_ref(z, z, z, np.ones(2), 0, A, count, 0.0, 0.0, 0.999, 1e-8, 0.0, max_grad_norm=max_norm)[1]
    assert _same(m[10:], (A[10:] / np.float64(count)) * scale) and not m[:10].any()
    got, rel = np.linalg.norm(m), clipped_norm_rel_bound(n_params - 10)
    print("n %d: |norm after the clip - max_norm| / max_norm %.3e, bound %.3e" % (n_params - 10, abs(got - max_norm) / max_norm, rel))
    assert abs(got - max_norm) <= rel * max_norm
    # the L2 term is added behind the clip: the same scale, whatever weight_decay is
    theta = np.random.default_rng(5).normal(size=n_params)
    m = P.fit_step_ref(theta, z, z, np.ones(2), 0, A, count, 0.0, 0.0, 0.999, 1e-8, 0.25, max_grad_norm=max_norm)[1]
    assert _same(m[10:], (A[10:] / np.float64(count)) * scale + np.float64(0.25) * theta[10:])


# ------------------------------------------------------------------------------------------------------------------ the rules
def test_argument_rules_need_no_device():
    nan, inf = float("nan"), float("inf")
    assert P.check_adv_normalize(7, 300, 303, 1e-8) == (7, 300, 303, 1e-8)
    assert P.check_adv_normalize(2 ** 15, 2 ** 16, 2 ** 16, 1e-8)[0] == 2 ** 15              # rows * stride == 2^31 is allowed
    for bad in ((0, 5, 5, 1e-8), (2, 0, 5, 1e-8), (2, 5, 4, 1e-8), (2 ** 15, 2 ** 16, 2 ** 16 + 1, 1e-8), (2, 5, 5, 0.0), (2, 5, 5, -1e-8),
                (2, 5, 5, nan), (2, 5, 5, inf), (True, 5, 5, 1e-8), (2.0, 5, 5, 1e-8)):
        with pytest.raises(ValueError):
            P.check_adv_normalize(*bad)
    assert P.adv_normalize_work_bytes(1) == 8 * 7 and P.adv_normalize_work_bytes(64) == 8 * 7 and P.adv_normalize_work_bytes(65) == 8 * 10
    assert P.adv_normalize_work_bytes(4097) == 8 * (4 + 3 * 65)
    with pytest.raises(ValueError):
        P.adv_normalize_work_bytes(0)
    assert P.check_max_grad_norm(0) == 0.0 and P.check_max_grad_norm(0.5) == 0.5
    for bad in (-0.5, nan, inf):
        with pytest.raises(ValueError):
            P.check_max_grad_norm(bad)
        with pytest.raises(ValueError):
            P.fit_step_ref(*_state(20, 0), np.zeros(20), 1, *ADAM, max_grad_norm=bad)
    with pytest.raises(ValueError):
        P.normalize_advantages(1, 2, 5, work=None)
    with pytest.raises(ValueError):
        P.normalize_advantages(1, 2, 5, work=1, eps=0.0)
    with pytest.raises(ValueError):
        P.adv_normalize_ref(np.zeros(5, np.float32))


def test_the_binding_declares_the_new_entry_points():
    lib = _lib.load()
    for name in ("bsk_adv_normalize_work_bytes", "bsk_adv_normalize", "bsk_fit_set_max_grad_norm", "bsk_fit_grad_norm_device",
                 "bsk_fit_apply_obs_norm"):
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.BSK_ABI_VERSION == 4
    for n in (1, 63, 64, 65, 300, 4097, 2 ** 28):
        assert lib.bsk_adv_normalize_work_bytes(n) == P.adv_normalize_work_bytes(n)
    assert lib.bsk_adv_normalize_work_bytes(0) == 0
    # the rules that need no device hold in the library before anything is launched
    assert lib.bsk_adv_normalize(None, None, 1, 1, 1, 1e-8, None, None, None) == -1
    assert lib.bsk_fit_set_max_grad_norm(None, 0.5) == -1 and lib.bsk_fit_grad_norm_device(None, None) == -1
    assert lib.bsk_fit_apply_obs_norm(None, None, 1e-6, None) == -1
