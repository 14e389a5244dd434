"""CPU: the numpy restatements behind the Adam update and the shared-episode reset of the device evolution strategy
(policy.es_tell_adam_ref, policy.shared_slot_ref; definitions in include/bskgpu.h), which tests/test_gpu_es_adam.py and
tests/test_gpu_es_shared.py then hold the kernels to bit for bit.

es_tell_adam_ref is compared BY BIT PATTERN with a restatement that shares nothing with it but the noise z (held to mpmath by
tests/test_es_host.py): plain Python loops over members, lanes and parameters, one `float` operation at a time - a Python float
is an IEEE double and every operator rounds once, which is what the header asks of the device.
"""
import ctypes
import math

import numpy as np
import pytest

from _policy_bounds import seeded_policy
from basilisk_env_amd import _lib
from basilisk_env_amd import policy as P
from basilisk_env_amd.envs.leoPowerAttitudeVecEnv import pool_slots

SEED = 2 ** 33 + 5
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _beats(a, ia, b, ib):
    na, nb = a != a, b != b
    if na != nb:
        return nb
    if not na and a != b:
        return a > b
    return ia < ib


def _loop_adam(theta, m, v, beta_pow, fitness, sigma, lr, frozen, seed, generation, beta1, beta2, eps, weight_decay):
    """include/bskgpu.h, tell under BSK_ES_ADAM, one operation at a time"""
    f = [float(x) for x in fitness]
    n_members, pairs, n = len(f), len(f) // 2, len(theta)
    rank = [sum(1 for t in range(n_members) if _beats(f[t], t, f[k], k)) for k in range(n_members)]
    u = [0.5 - float(r) / float(max(n_members - 1, 1)) for r in rank]
    w = [u[2 * i] - u[2 * i + 1] for i in range(pairs)]
    z = P.es_noise_ref(seed, generation, pairs, n).tolist()
    theta, m, v = [float(x) for x in theta], [float(x) for x in m], [float(x) for x in v]
    cg = 1.0 / (float(n_members) * sigma)
    a1, a2 = 1.0 - beta1, 1.0 - beta2
    p1, p2 = float(beta_pow[0]) * beta1, float(beta_pow[1]) * beta2
    for j in range(frozen, n):
        s = [0.0] * 64
        for lane in range(64):
            for i in range(lane, pairs, 64):
                t = w[i] * z[i][j]
                s[lane] = t if i == lane else s[lane] + t
        stride = 32
        while stride:
            for lane in range(stride):
                s[lane] = s[lane] + s[lane + stride]
            stride //= 2
        g = cg * s[0] - weight_decay * theta[j]
        m[j] = beta1 * m[j] + a1 * g
        v[j] = beta2 * v[j] + (a2 * g) * g
        theta[j] = theta[j] + (lr * (m[j] / (1.0 - p1))) / (math.sqrt(v[j] / (1.0 - p2)) + eps)
    return np.array(theta), np.array(m), np.array(v), np.array([p1, p2])


def _fitness(n_members, generation):
    """ties, a NaN, +-inf; another vector every generation"""
    if n_members == 2:
        return np.array([[1.0, 1.0], [np.nan, 0.0], [-np.inf, np.inf], [0.25, -3.0]][generation])
    f = np.random.default_rng(100 * n_members + generation).normal(size=n_members)
    f[7] = f[3]
    f[10] = f[11] = np.nan
    f[20], f[21], f[40], f[41 + 64] = np.inf, -np.inf, np.inf, np.nan
    return f if generation % 2 == 0 else np.roll(f, generation)


@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
@pytest.mark.parametrize("frozen", [0, 10])
@pytest.mark.parametrize("n_members", [2, 130, 256])
def test_adam_ref_equals_the_loop_restatement_bit_for_bit(n_members, frozen, weight_decay):
    _, theta0 = seeded_policy((16,), "relu", None, seed=9)
    sigma, lr = 0.1, 0.05
    a = (theta0.astype(np.float64), np.zeros(theta0.size), np.zeros(theta0.size), np.ones(2))
    b = a
    for generation in range(4):
        f = _fitness(n_members, generation)
        a = P.es_tell_adam_ref(*a, f, sigma, lr, frozen, SEED, generation, BETA1, BETA2, EPS, weight_decay)
        b = _loop_adam(*b, f, sigma, lr, frozen, SEED, generation, BETA1, BETA2, EPS, weight_decay)
        for x, y, name in zip(a, b, ("theta", "m", "v", "beta_pow")):
            assert x.dtype == np.float64 and np.array_equal(_bits(x), _bits(y)), (generation, name)
        assert np.isfinite(a[0]).all()
    theta, m, v, beta_pow = a
    assert np.array_equal(_bits(theta[:frozen]), _bits(theta0[:frozen])) and not m[:frozen].any() and not v[:frozen].any()
    assert m[frozen:].any() and (v[frozen:] > 0.0).all() and not np.array_equal(theta[frozen:], theta0[frozen:])
    assert np.array_equal(_bits(beta_pow), _bits([BETA1 * BETA1 * BETA1 * BETA1, BETA2 * BETA2 * BETA2 * BETA2]))
    # the inputs are not written to
    assert np.array_equal(_bits(theta0), _bits(seeded_policy((16,), "relu", None, seed=9)[1]))


def test_tell_ref_still_takes_its_sum_from_the_shared_code():
    """es_tell_ref's result is lr / (P sigma) times the sum es_tell_adam_ref's gradient is made of"""
    _, theta0 = seeded_policy((16,), "relu", None, seed=9)
    f = _fitness(130, 0)
    s0, n_members = P._es_pair_sum(f, theta0.size, SEED, 3)
    theta = theta0.astype(np.float64)
    want = theta.copy()
    want[10:] = want[10:] + (0.05 / (130.0 * 0.1)) * s0[10:]
    assert n_members == 130 and np.array_equal(_bits(P.es_tell_ref(theta0, f, 0.1, 0.05, 10, SEED, 3)), _bits(want))


def test_first_step_from_zero_moments_is_lr_times_g_over_g_plus_eps():
    """m / (1 - beta1) = g and v / (1 - beta2) = g^2 after one step from zero, up to rounding: the step is lr g / (|g| + eps), at
    most lr.  The bias corrections swapped would make it a thousand times lr.  Eight roundings of 2^-53 each: 1e-14 relative."""
    _, theta0 = seeded_policy((16,), "relu", None, seed=9)
    n, n_members, sigma, lr, frozen = theta0.size, 130, 0.1, 0.05, 10
    f = np.random.default_rng(3).normal(size=n_members)
    theta, m, v, beta_pow = P.es_tell_adam_ref(theta0, np.zeros(n), np.zeros(n), np.ones(2), f, sigma, lr, frozen, SEED, 0, BETA1, BETA2,
                                               EPS, 0.0)
    s0, _ = P._es_pair_sum(f, n, SEED, 0)
    g = s0[frozen:] / (n_members * sigma)
    step = theta[frozen:] - theta0[frozen:].astype(np.float64)
    assert (np.abs(step) <= lr).all() and (np.abs(step) > 0.99 * lr).sum() > 100
    want = lr * g / (np.abs(g) + EPS)
    # (theta + step - theta loses the bits of step below an ulp of theta: |theta| < 8, so 2^-50 absolute)
    assert np.abs(step - want).max() <= 1e-14 * lr + 2.0 ** -50
    assert np.array_equal(np.sign(step), np.sign(g)) and np.array_equal(_bits(beta_pow), _bits([BETA1, BETA2]))


def test_two_hundred_generations_descend_on_the_quadratic():
    n_members, sigma, lr, frozen, seed = 16, 0.1, 0.05, 10, 11
    _, theta0 = seeded_policy((16,), "relu", None, seed=13)
    n = theta0.size
    target = np.concatenate([theta0[:frozen].astype(np.float64), np.random.default_rng(4).normal(size=n - frozen)])
    state = (theta0.astype(np.float64), np.zeros(n), np.zeros(n), np.ones(2))
    for g in range(200):
        members = P.es_ask_ref(state[0], sigma, frozen, n_members, seed, g)
        fitness = -((members.astype(np.float64) - target) ** 2).sum(axis=1)
        state = P.es_tell_adam_ref(*state, fitness, sigma, lr, frozen, seed, g, BETA1, BETA2, EPS, 0.0)
    start, end = np.linalg.norm(theta0 - target), np.linalg.norm(state[0] - target)
    assert end < 0.5 * start, (start, end)
    assert np.array_equal(_bits(state[0][:frozen]), _bits(theta0[:frozen]))


# (n = 200, E = 48, n_pool = 41): the first eight slots per (env_base, epoch), from the header's formula in Python integers
PINNED = {
    (0, 0): [4, 30, 19, 4, 34, 23, 8, 38], (0, 1): [40, 25, 14, 40, 29, 18, 3, 33], (0, 2 ** 32 + 3): [30, 15, 4, 30, 19, 8, 34, 23],
    (70, 0): [13, 2, 28, 17, 6, 32, 21, 6], (70, 1): [8, 38, 23, 12, 1, 27, 16, 1], (70, 2 ** 32 + 3): [39, 28, 13, 2, 32, 17, 6, 32],
    (128, 0): [10, 40, 29, 14, 3, 29, 18, 7], (128, 1): [5, 35, 24, 9, 39, 24, 13, 2], (128, 2 ** 32 + 3): [36, 25, 14, 40, 29, 14, 3, 33],
}


def _slot_int(env, env_base, E, epoch, n_pool):
    q = ((env + env_base) & 0xFFFFFFFF) % E
    return ((q * 2654435761 + (epoch & 0xFFFFFFFF) * 40503 + 12345) & 0xFFFFFFFF) % n_pool


@pytest.mark.parametrize("env_base", [0, 70, 128])
@pytest.mark.parametrize("epoch", [0, 1, 2 ** 32 + 3])
def test_shared_slots_are_the_header_formula(epoch, env_base):
    n, E, n_pool = 200, 48, 41
    slots = P.shared_slot_ref(n, E, epoch, n_pool, env_base)
    assert slots.dtype == np.uint32 and slots.shape == (n,)
    assert slots.tolist() == [_slot_int(j, env_base, E, epoch, n_pool) for j in range(n)]
    assert slots[:8].tolist() == PINNED[(env_base, epoch)]
    # equal q, equal slot - and the slots of one member are not all one
    q = (np.arange(n) + env_base) % E
    for j in range(n):
        assert slots[j] == slots[np.flatnonzero(q == q[j])[0]]
    assert len(set(slots[:E].tolist())) > 20
    # a new epoch draws anew; the high word of the epoch is not read
    assert not np.array_equal(slots, P.shared_slot_ref(n, E, epoch + 1, n_pool, env_base))
    assert np.array_equal(slots, P.shared_slot_ref(n, E, epoch + 2 ** 32, n_pool, env_base))


def test_shared_slots_meet_the_per_env_rule_where_no_index_wraps():
    """envs_per_member above every global index: q = g, and under epoch 0 the rule is the auto-reset's at episode 0"""
    for n, env_base, n_pool in ((200, 0, 41), (200, 70, 41), (64, 128, 7)):
        want = pool_slots(np.arange(n) + env_base, np.zeros(n, np.int64), n_pool)
        assert np.array_equal(P.shared_slot_ref(n, env_base + n + 1, 0, n_pool, env_base).astype(np.int64), want)
        assert not np.array_equal(P.shared_slot_ref(n, 48, 0, n_pool, env_base).astype(np.int64), want)
    # the global index is 32 bits wide, as in the kernels
    assert np.array_equal(P.shared_slot_ref(4, 48, 0, 41, 2 ** 32 - 2), [_slot_int(j, 2 ** 32 - 2, 48, 0, 41) for j in range(4)])
    with pytest.raises(ValueError):
        P.shared_slot_ref(4, 0, 0, 41)


NAN, INF = float("nan"), float("inf")
REFUSED = ([dict(beta1=b) for b in (-0.1, 1.0, 1.5, NAN, INF)] + [dict(beta2=b) for b in (-0.1, 1.0, NAN, -INF)] +
           [dict(eps=e) for e in (0.0, -1e-8, NAN, INF)] + [dict(weight_decay=d) for d in (-1e-3, NAN, INF)])


@pytest.mark.parametrize("bad", REFUSED, ids=lambda d: "%s=%r" % next(iter(d.items())))
def test_python_refuses_what_set_optimizer_refuses(bad):
    spec, theta0 = seeded_policy((16,), "relu", None, seed=9)
    args = dict(beta1=BETA1, beta2=BETA2, eps=EPS, weight_decay=0.0)
    assert P.check_adam(**args) == (BETA1, BETA2, EPS, 0.0) and P.check_adam(0.0, 0.0, 1e-300, 0.0) == (0.0, 0.0, 1e-300, 0.0)
    args.update(bad)
    with pytest.raises(ValueError):
        P.check_adam(**args)
    with pytest.raises(ValueError):                       # before the library is asked for an optimiser: no device needed
        P.DeviceEvolutionStrategy(spec, theta0, 4, optimizer="adam", **bad)
    with pytest.raises(ValueError):
        P.es_tell_adam_ref(theta0, np.zeros(theta0.size), np.zeros(theta0.size), np.ones(2), np.zeros(4), 0.1, 0.05, 10, 0, 0,
                           args["beta1"], args["beta2"], args["eps"], args["weight_decay"])


def test_python_refuses_an_unknown_optimizer():
    spec, theta0 = seeded_policy((16,), "relu", None, seed=9)
    for kind in ("rmsprop", "ADAM", 1, None):
        with pytest.raises(ValueError):
            P.DeviceEvolutionStrategy(spec, theta0, 4, optimizer=kind)


def test_the_library_exports_the_new_entry_points_and_refuses_null():
    lib = _lib.load()
    for name in ("bsk_reset_from_pool_shared", "bsk_es_generation_device", "bsk_es_set_optimizer", "bsk_es_get_moments", "bsk_es_set_moments"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    p = ctypes.c_void_p()
    assert lib.bsk_reset_from_pool_shared(None, 64, None, None) == -1 and b"NULL" in lib.bsk_last_error()
    assert lib.bsk_es_generation_device(None, ctypes.byref(p)) == -1
    assert lib.bsk_es_set_optimizer(None, _lib.ES_ADAM, BETA1, BETA2, EPS, 0.0) == -1
    assert lib.bsk_es_get_moments(None, None, None, None) == -1 and lib.bsk_es_set_moments(None, None, None, None) == -1
    assert (_lib.ES_SGD, _lib.ES_ADAM) == (0, 1)
