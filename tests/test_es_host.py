"""CPU: the numpy restatement of the device evolution strategy (policy.es_noise_ref / es_ask_ref / es_tell_ref; definition in
include/bskgpu.h) - its inverse normal CDF against mpmath, the distribution of its draws, and the update against the plain
matrix product and against EvolutionStrategy.  tests/test_gpu_es.py holds the kernels to these functions bit for bit.

The reference for the inverse normal CDF is one Newton step from the value under test, in 40-digit mpmath:
z* = z - (Phi(z) - u) / phi(z) with u = (k + 0.5) * 2**-52 exact.  |z - z*| <= 1e-14 here, so the step's own error, about
|z| / 2 * (z - z*)**2 < 1e-27, is far below what is measured.
"""
import mpmath as mp
import numpy as np
import pytest

from _es_cases import TAIL_K_FAR, beyond_one_tile, tail_rows
from basilisk_env_amd import policy as P

# The greatest errors measured over the sample of _sample_k() (they are printed by the test): 4.1e-15 absolute, 7.1e-16 relative.
# The bounds are four times that, the margin for points the sample missed.
MEASURED_ABS, MEASURED_REL = 4.1e-15, 7.1e-16
BOUND_ABS, BOUND_REL = 4 * MEASURED_ABS, 4 * MEASURED_REL


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _switch(pred, lo, hi):
    """pred(lo) true, pred(hi) false, monotone in between -> the last k where it holds"""
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


def _u(k):
    return P.es_uniform_ref(np.array([k], np.uint64))


def _sample_k():
    ks = [0, 1, 2, 2 ** 51 - 1, 2 ** 51, 2 ** 52 - 1]
    # the u nearest either side of |q| = 0.425 (the centre's rational against the tail's) ...
    a = _switch(lambda k: abs(float(_u(k)[0]) - 0.5) > 0.425, 0, 2 ** 51)
    # ... and of r = 5 (the two tail rationals), in the lower and - mirrored - the upper tail
    b = _switch(lambda k: float(np.sqrt(-P._series_log(_u(k)))[0]) > 5.0, 0, a)
    assert 0 < b < a < 2 ** 51 and abs(b / 2.0 ** 52 / np.exp(-25.0) - 1) < 1e-3 and abs(a / 2.0 ** 52 - 0.075) < 1e-9
    for k in (a, a + 1, b, b + 1):
        ks += [k, 2 ** 52 - 1 - k]
    ks += np.unique(np.round(np.logspace(0, np.log10(2.0 ** 52 - 1), 4000)).astype(np.uint64)).tolist()
    ks += np.random.default_rng(1).integers(0, 2 ** 52, 20000, dtype=np.uint64).tolist()
    return np.array(ks, np.uint64)


@pytest.fixture(scope="module")
def sample():
    k = _sample_k()
    return k, P.es_inverse_normal_ref(P.es_uniform_ref(k))


def test_inverse_normal_against_mpmath(sample):
    k, z = sample
    mp.mp.dps = 40
    err = rel = mp.mpf(0)
    for ki, zi in zip(k.tolist(), z.tolist()):
        u = (mp.mpf(ki) + mp.mpf("0.5")) * mp.mpf(2) ** -52
        d = abs((mp.ncdf(zi) - u) / mp.npdf(zi))
        err, rel = max(err, d), max(rel, d / abs(mp.mpf(zi) - d))
    print("inverse normal CDF against mpmath over %d points: %.3g absolute, %.3g relative" % (k.size, float(err), float(rel)))
    assert BOUND_ABS <= 1e-12                  # (sigma * 1e-12 is far below one float32 ulp of any member)
    assert float(err) <= BOUND_ABS and float(rel) <= BOUND_REL
    assert np.isfinite(z).all() and abs(z[0] + 8.2095) < 1e-4 and z[0] == z.min() and z[5] == z.max()


def test_inverse_normal_is_antisymmetric_to_the_bit(sample):
    k, z = sample
    mirrored = P.es_inverse_normal_ref(P.es_uniform_ref(np.uint64(2 ** 52 - 1) - k))
    assert np.array_equal(_bits(mirrored), _bits(-z))
    assert np.array_equal(P.es_uniform_ref(np.uint64(2 ** 52 - 1) - k), 1.0 - P.es_uniform_ref(k))      # 1 - u is exact


def test_the_recorded_seeds_draw_from_the_far_tail():
    """The far branch of the inverse normal CDF (r > 5, the E / F rationals) through the whole chain seed -> Philox -> k -> u -> z:
    tests/test_gpu_es.py asks the device for the z recorded here, so the record is held to the restatement's bits, to the branch
    (|z| above the E polynomial's value at r = 5, which the r <= 5 branch never exceeds) and to mpmath."""
    rows, k_far = tail_rows(), TAIL_K_FAR
    assert len(rows) >= 3 and any(seed >= 2 ** 32 for seed, _, _, _ in rows)         # (the key's high word)
    assert any(z > 0 for _, _, _, z in rows) and any(z < 0 for _, _, _, z in rows)
    mp.mp.dps = 40
    for seed, j, k, z in rows:
        got = P.es_noise_ref(seed, 0, 1, j + 1)[0, j]
        assert np.array_equal(_bits(got), _bits(z)), (seed, j, float(got).hex())
        # the k of the definition, and on the far side of the switch test_inverse_normal_against_mpmath's sample finds by bisection
        w0, w1, _, _ = P.philox4x32_10(j, 0, 0, 0, seed & 0xFFFFFFFF, seed >> 32)
        assert (int(w0) >> 6) * 2 ** 26 + (int(w1) >> 6) == k and min(k, 2 ** 52 - 1 - k) <= k_far
        assert _bits(P.es_inverse_normal_ref(_u(k)))[0] == _bits(z)[0]
        assert float(np.sqrt(-P._series_log(_u(min(k, 2 ** 52 - 1 - k))))[0]) > 5.0
        assert abs(z) > 6.6579046435 and (z < 0) == (k < 2 ** 51)
        u = (mp.mpf(k) + mp.mpf("0.5")) * mp.mpf(2) ** -52
        want = mp.sqrt(2) * mp.erfinv(2 * u - 1)
        d = abs(mp.mpf(z) - want)
        print("seed %d, j %d: z %s, |z - mpmath| %.3g" % (seed, j, float(z).hex(), float(d)))
        assert float(d) <= BOUND_ABS and float(d / abs(want)) <= BOUND_REL


def test_moments_of_two_million_draws():
    z = P.es_noise_ref(20260, 3, 1000, 2000).ravel()
    n = z.size
    assert n == 2 * 10 ** 6
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2
    print("mean %.3g, variance %.6f, kurtosis %.5f" % (mean, var, kurt))
    assert abs(mean) <= 5 * np.sqrt(1.0 / n) and abs(var - 1) <= 5 * np.sqrt(2.0 / n) and abs(kurt - 3) <= 5 * np.sqrt(24.0 / n)


def test_noise_depends_on_every_word_of_its_counter_and_key():
    base = P.es_noise_ref(5, 7, 3, 4)
    assert base.shape == (3, 4) and len(set(base.ravel().tolist())) == 12
    for seed, g in ((5 + 2 ** 32, 7), (5, 7 + 2 ** 32), (6, 7), (5, 8)):
        assert not np.array_equal(P.es_noise_ref(seed, g, 3, 4), base)
    assert np.array_equal(P.es_noise_ref(5, 7, 2, 3), base[:2, :3])        # (pair, parameter) address the draw, not the shape


def test_ask_is_antithetic_and_leaves_the_frozen_entries():
    theta = np.random.default_rng(2).normal(size=23)
    m = P.es_ask_ref(theta, 0.25, 10, 6, 9, 4)
    z = P.es_noise_ref(9, 4, 3, 23)
    assert m.dtype == np.float32 and m.shape == (6, 23)
    assert np.array_equal(m[:, :10], np.broadcast_to(theta[:10].astype(np.float32), (6, 10)))
    assert np.array_equal(m[0::2, 10:], (theta[10:] + 0.25 * z[:, 10:]).astype(np.float32))
    assert np.array_equal(m[1::2, 10:], (theta[10:] - 0.25 * z[:, 10:]).astype(np.float32))
    assert np.array_equal(P.es_ask_ref(theta, 0.25, 0, 6, 9, 4)[0::2], (theta + 0.25 * z).astype(np.float32))


@pytest.mark.parametrize("n_members", [2, 16, 130, 256, 1024])
def test_tell_against_the_plain_product_and_the_host_strategy(n_members):
    rng = np.random.default_rng(n_members)
    n, frozen, seed, g = 57, 10, 2 ** 33 + 5, 2
    fitness = rng.normal(size=n_members)
    z = P.es_noise_ref(seed, g, n_members // 2, n)
    u = P.centred_ranks(fitness)
    # c = lr / (P * sigma) = 1 exactly and theta = 0: what tell returns is the ordered sum itself
    step = P.es_tell_ref(np.zeros(n), fitness, 0.5, 0.5 * n_members, frozen, seed, g)
    plain = (u[0::2] - u[1::2]) @ z
    assert not step[:frozen].any() and step[frozen:].all()
    assert np.abs(step[frozen:] - plain[frozen:]).max() <= 1e-12 * np.abs(plain[frozen:]).max()
    # EvolutionStrategy.tell fed the same noise
    theta = rng.normal(size=n)
    host = P.EvolutionStrategy(theta, n_members, sigma=0.1, lr=0.05, seed=0, frozen=frozen)
    host.ask()
    host._eps = z.copy()
    host._eps[:, :frozen] = 0.0
    host.tell(fitness)
    ours = P.es_tell_ref(theta, fitness, 0.1, 0.05, frozen, seed, g)
    assert np.array_equal(_bits(ours[:frozen]), _bits(theta[:frozen]))
    assert np.abs(ours - host.theta).max() <= 1e-12 * np.abs(host.theta).max()
    assert np.abs((ours - theta) - (host.theta - theta))[frozen:].max() <= 1e-12 * np.abs(host.theta - theta).max()


def _ranks_by_counting(f):
    """the device's rule, restated on its own: rank_k = how many members beat member k (bsk_select_branches' beats)"""
    def beats(a, ia, b, ib):
        na, nb = a != a, b != b
        if na != nb:
            return nb
        if not na and a != b:
            return a > b
        return ia < ib
    P_ = len(f)
    rank = [sum(beats(f[m], m, f[k], k) for m in range(P_)) for k in range(P_)]
    return 0.5 - np.array(rank, np.float64) / max(P_ - 1, 1)


@pytest.mark.parametrize("fitness", [
    [1.0, 1.0], [3.0, -np.inf, np.nan, 3.0, np.inf, np.nan, 0.0, -0.0], [np.nan] * 4, [np.inf, np.inf, -np.inf, -np.inf],
    [0.5, 2.0, 2.0, 2.0, -1.0, np.nan, np.inf, 0.5, 0.5, -np.inf]], ids=["tie", "mixed", "nan", "inf", "ties"])
def test_ties_nan_and_infinities_rank_as_centred_ranks(fitness):
    f = np.array(fitness, np.float64)
    u = P.centred_ranks(f)
    assert np.array_equal(_bits(_ranks_by_counting(f)), _bits(u))
    assert sorted(u.tolist()) == sorted((0.5 - np.arange(f.size) / max(f.size - 1, 1)).tolist())
    theta = np.linspace(-1, 1, 14)
    got = P.es_tell_ref(theta, f, 0.1, 0.05, 3, 1, 0)
    z = P.es_noise_ref(1, 0, f.size // 2, 14)
    want = theta + 0.05 / (f.size * 0.1) * ((u[0::2] - u[1::2]) @ z)
    assert np.isfinite(got).all() and np.array_equal(got[:3], theta[:3]) and np.allclose(got, np.where(np.arange(14) < 3, theta, want), rtol=0, atol=1e-13)


def test_the_vectors_beyond_one_tile_rank_as_the_counting_rule_says():
    """tests/_es_cases.py: what the GPU tests feed the ranking kernels at 258 members, against the counting rule restated above"""
    cases = beyond_one_tile(258, np.random.default_rng(258))
    assert len(cases) == 4 and beyond_one_tile(256, np.random.default_rng(0)) == []
    a, b, c, d = cases
    assert a[257] == a[5] and np.isnan(a[256]) and np.isnan(b[[11, 256, 257]]).all() and c[256] == c[257] == c.max()
    assert d[256] == np.inf and d[257] == -np.inf
    ranks = []
    for f in cases:
        u = P.centred_ranks(f)
        assert np.array_equal(_bits(_ranks_by_counting(f)), _bits(u))
        ranks.append(np.rint((0.5 - u) * 257).astype(int))
    assert ranks[0][257] == ranks[0][5] + 1 and ranks[0][256] == 257      # the tie goes to the lower index; the one NaN is last
    assert ranks[1][[11, 256, 257]].tolist() == [255, 256, 257]           # the three NaNs at the bottom, by index
    assert ranks[2][[256, 257]].tolist() == [0, 1] and ranks[3][[40, 256, 257]].tolist() == [0, 1, 257]


def test_tell_refuses_odd_and_empty_populations():
    for f in ([], [1.0], [1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):
            P.es_tell_ref(np.zeros(4), f, 0.1, 0.05, 0, 0, 0)


def test_sixty_generations_descend_on_a_quadratic():
    rng = np.random.default_rng(4)
    n, n_members, frozen, sigma, lr, seed = 40, 16, 10, 0.1, 0.05, 11
    theta0 = np.concatenate([rng.normal(size=frozen), np.zeros(n - frozen)])
    target = np.concatenate([theta0[:frozen], rng.normal(size=n - frozen)])
    theta = theta0.copy()
    for g in range(60):
        members = P.es_ask_ref(theta, sigma, frozen, n_members, seed, g).astype(np.float64)
        theta = P.es_tell_ref(theta, -((members - target) ** 2).sum(axis=1), sigma, lr, frozen, seed, g)
    start, end = np.linalg.norm(theta0 - target), np.linalg.norm(theta - target)
    print("distance to the target: %.4f -> %.4f" % (start, end))
    assert end < 0.5 * start
    assert np.array_equal(_bits(theta[:frozen]), _bits(theta0[:frozen]))


def test_the_binding_tracks_the_new_entry_points():
    from basilisk_env_amd import _lib
    lib = _lib.load()
    for name in ("bsk_es_create", "bsk_es_destroy", "bsk_es_ask", "bsk_es_tell", "bsk_es_get_state", "bsk_es_set_state"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    # the argument rules come before the device: refused here, where there is none, for the right reason
    import ctypes
    spec, h = P.c_spec(P.check_spec((16,), "relu")), ctypes.c_void_p()
    for args in ((3, 0.1, 0.05, 10), (0, 0.1, 0.05, 10), (65538, 0.1, 0.05, 10), (4, 0.0, 0.05, 10), (4, -1.0, 0.05, 10),
                 (4, float("nan"), 0.05, 10), (4, float("inf"), 0.05, 10), (4, 0.1, float("nan"), 10), (4, 0.1, float("inf"), 10),
                 (4, 0.1, 0.05, -1), (4, 0.1, 0.05, P.n_params(P.check_spec((16,), "relu")) + 1)):
        assert lib.bsk_es_create(ctypes.byref(spec), args[0], None, args[1], args[2], args[3], 0, 0, ctypes.byref(h)) == -1, args
        assert lib.bsk_last_error() and not h.value
    assert lib.bsk_es_create(None, 4, None, 0.1, 0.05, 10, 0, 0, ctypes.byref(h)) == -1
    assert lib.bsk_es_create(ctypes.byref(spec), 4, None, 0.1, 0.05, 10, 0, 0, None) == -1
    assert lib.bsk_es_ask(None, None, None) == -1 and lib.bsk_es_tell(None, None, None) == -1
    assert lib.bsk_es_get_state(None, None, None) == -1 and lib.bsk_es_set_state(None, None, 0) == -1
