"""CPU, no library: the numpy restatements of the running observation statistics (policy_ref.obs_stats_accumulate_ref,
obs_stats_totals_ref, obs_norm_ref; definition in include/bskgpu.h) - what tests/test_gpu_obs_stats.py holds the kernels to bit for bit.

The sums are held to exact rational arithmetic (fractions.Fraction) on the same inputs under the standard bound of a summation
whose elements pass through at most m additions (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2):
    |computed - exact| <= gamma_m * sum |x_i|,   gamma_m = m u / (1 - m u),   u = 2^-53.
m is derived here from the order the definition fixes.  An element accumulated in call c of C, with W partial rows, passes through
    6 additions of the wave's tree,
    C - c + 1 additions into part[w] (its own call's and every later one's),
    ceil(W / 64) - 1 additions at most along its lane of the join,
    6 additions of the join's tree:
m = 6 + C + (ceil(W / 64) - 1) + 6 for the sums.  A sum of squares carries one more rounding per element, that of x * x: m + 1.
"""
from fractions import Fraction

import numpy as np
import pytest

from basilisk_env_amd import policy as P
from basilisk_env_amd import policy_ref as R

U = Fraction(1, 2 ** 53)


def _gamma(m):
    return m * U / (1 - m * U)


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.int64)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _block(rng, n):
    """(5, n) float64 of either sign with magnitudes spread over 1e-6 .. 1e3"""
    return np.where(rng.random((5, n)) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-6.0, 3.0, (5, n))


def test_the_public_names_are_re_exported():
    for name in ("obs_stats_accumulate_ref", "obs_stats_totals_ref", "obs_norm_ref", "obs_stats_zero_state", "obs_moments_ref"):
        assert getattr(P, name) is getattr(R, name)


@pytest.mark.parametrize("n,n_cap,masked", [(64, 64, False), (100, 200, True), (8320, 8320, True), (4097, 4200, False)])
def test_sums_stay_within_the_bound_of_their_depth(n, n_cap, masked):
    rng = np.random.default_rng(n)
    state = R.obs_stats_zero_state(n_cap)
    W = state[0].shape[0]
    assert W == (n_cap + 63) // 64
    calls = 3
    m = 6 + calls + ((W + 63) // 64 - 1) + 6
    exact = [Fraction(0)] * 10
    mass = [Fraction(0)] * 10
    count = 0
    for c in range(calls):
        obs = _block(rng, n)
        alive = None
        if masked:
            alive = (rng.random(n) < 0.7).astype(np.uint8)
            alive[64 * (c % ((n + 63) // 64)):][:64] = 0          # one wholly dead wave, another one in every call
        before, kept = state, (state[0].copy(), state[1].copy())
        state = R.obs_stats_accumulate_ref(before, obs, alive)
        assert _same(before[0], kept[0]) and np.array_equal(before[1], kept[1])          # (the input state is not changed)
        use = np.ones(n, bool) if alive is None else alive != 0
        count += int(use.sum())
        for k in range(5):
            xs = [Fraction(float(v)) for v in obs[k, use]]
            exact[k] += sum(xs)
            exact[5 + k] += sum(x * x for x in xs)
            mass[k] += sum(abs(x) for x in xs)
            mass[5 + k] += sum(x * x for x in xs)
        tot, got_count = R.obs_stats_totals_ref(state)
        assert got_count == count == int(state[1].sum())
        for col in range(10):
            depth = m if col < 5 else m + 1
            err = abs(Fraction(float(tot[col])) - exact[col])
            assert err <= _gamma(depth) * mass[col], (c, col, float(err), float(_gamma(depth) * mass[col]))
    # per wave: the count is the number of counting lanes, and a wave that never counted was never stored to
    assert int(state[1][(n + 63) // 64:].sum()) == 0 and not state[0][(n + 63) // 64:].any()


def test_two_calls_equal_one_state_carried_through_both():
    rng = np.random.default_rng(3)
    n = 200
    a, b = _block(rng, n), _block(rng, n)
    alive = (rng.random(n) < 0.5).astype(np.uint8)
    zero = R.obs_stats_zero_state(n)
    s1 = R.obs_stats_accumulate_ref(zero, a, None)
    s2 = R.obs_stats_accumulate_ref(s1, b, alive)
    # the same two blocks through a state that went to the host and back in between (a checkpoint)
    carried = (np.array(s1[0].tolist()), np.array(s1[1].tolist(), dtype=np.uint64))
    t2 = R.obs_stats_accumulate_ref(carried, b, alive)
    assert _same(s2[0], t2[0]) and np.array_equal(s2[1], t2[1])
    assert not zero[0].any() and not zero[1].any()
    # per wave the rule is part = part + wave sum: the second call alone, added by hand
    alone = R.obs_stats_accumulate_ref(zero, b, alive)
    assert _same(s2[0], s1[0] + alone[0]) and np.array_equal(s2[1], s1[1] + alone[1])
    # a shorter block leaves the waves beyond it alone
    s3 = R.obs_stats_accumulate_ref(s2, a[:, :70], None)
    assert _same(s3[0][2:], s2[0][2:]) and np.array_equal(s3[1], s2[1] + np.array([64, 6, 0, 0], np.uint64))
    for bad in (np.zeros((5, 0)), np.zeros((4, 8)), np.zeros((5, 257))):
        with pytest.raises(ValueError):
            R.obs_stats_accumulate_ref(zero, bad, None)
    with pytest.raises(ValueError):
        R.obs_stats_accumulate_ref(zero, a, alive[:-1])


def test_signed_zeros_and_lanes_without_a_partial():
    neg = np.full((5, 64), -0.0)
    part, cnt = R.obs_stats_accumulate_ref(R.obs_stats_zero_state(64), neg, None)
    # -0.0 + -0.0 = -0.0 down the tree, then part = +0.0 + -0.0 = +0.0; the squares are +0.0 throughout
    assert _same(part, np.zeros((1, 10))) and cnt.tolist() == [64]
    # one dead lane brings +0.0 into the tree: the same +0.0
    alive = np.ones(64, np.uint8)
    alive[5] = 0
    part, cnt = R.obs_stats_accumulate_ref(R.obs_stats_zero_state(64), neg, alive)
    assert _same(part, np.zeros((1, 10))) and cnt.tolist() == [63]
    # a wave in which nothing counts stores nothing: a -0.0 that a checkpoint put there stays (+0.0 would have been added otherwise)
    state = (np.full((2, 10), -0.0), np.zeros(2, np.uint64))
    part, cnt = R.obs_stats_accumulate_ref(state, np.ones((5, 128)), np.r_[np.zeros(64, np.uint8), np.ones(64, np.uint8)])
    assert _same(part[0], np.full(10, -0.0)) and _same(part[1], np.full(10, 64.0)) and cnt.tolist() == [0, 64]
    # a dead lane's value is never looked at: a NaN there does not reach the sums
    obs = np.ones((5, 64))
    obs[:, 5] = np.nan
    part, _ = R.obs_stats_accumulate_ref(R.obs_stats_zero_state(64), obs, alive)
    assert _same(part[0], np.full(10, 63.0))
    # the join: lanes 1 .. 63 of one partial row hold +0.0, so a -0.0 total cannot survive the tree; with 65 rows lane 0 has two
    tot, count = R.obs_stats_totals_ref((np.full((1, 10), -0.0), np.array([7], np.uint64)))
    assert _same(tot, np.zeros(10)) and count == 7
    tot, _ = R.obs_stats_totals_ref((np.full((64, 10), -0.0), np.zeros(64, np.uint64)))
    assert _same(tot, np.full(10, -0.0))                     # (every lane holds its first element, not zero + it)
    part = np.zeros((65, 10))
    part[0], part[64], part[3] = 1.0, 2.0 ** -53, 2.0 ** -53
    tot, _ = R.obs_stats_totals_ref((part, np.zeros(65, np.uint64)))
    # lane 0 adds 1 + 2^-53 first (ties to even: 1), then the tree brings lane 3's 2^-53 (1 again); one sum of all three gives more
    assert _same(tot, np.full(10, 1.0)) and 1.0 + (2.0 ** -53 + 2.0 ** -53) > 1.0
    # a count beyond 2^53 is summed in integers
    _, count = R.obs_stats_totals_ref((np.zeros((2, 10)), np.array([2 ** 60 + 1, 2 ** 60 + 1], np.uint64)))
    assert count == 2 ** 61 + 2


def test_the_normalisation_and_its_edges():
    # nothing counted: nothing is written
    assert R.obs_norm_ref(np.zeros(10), 0, 1e-6) is None
    # four rows of known moments and a constant fifth
    N = 4
    rows = np.array([[1.0, 2.0, 3.0, 6.0], [-2.0, -2.0, 2.0, 2.0], [0.5, 0.5, 0.5, 1.5], [1e3, -1e3, 1e3, -1e3], [0.25] * 4])
    tot = np.r_[rows.sum(axis=1), (rows * rows).sum(axis=1)]
    mean, var = R.obs_moments_ref(tot, N)
    assert _same(mean, [3.0, 0.0, 0.75, 0.0, 0.25]) and _same(var, [3.5, 4.0, 0.1875, 1e6, 0.0])
    scale, shift = R.obs_norm_ref(tot, N, 1e-6)
    sd = np.sqrt(var)
    assert _same(scale[:4], 1.0 / sd[:4]) and _same(shift[:4], 0.0 - mean[:4] * scale[:4])
    # the constant row is switched off: scale = +0.0, and shift = 0.0 - 0.25 * 0.0 = 0.0 - 0.0 = +0.0
    assert _same(scale[4:], [0.0]) and _same(shift[4:], [0.0])
    # ... with a negative mean the product is -0.0 and 0.0 - -0.0 is +0.0 as well; a zero mean under a live scale gives 0.0 - 0.0
    s2, h2 = R.obs_norm_ref(np.r_[[-1.0] * 5, [0.25] * 5], N, 1e-6)
    assert _same(s2, np.zeros(5)) and _same(h2, np.zeros(5))
    assert _same(shift[1:2], [0.0]) and _same(shift[3:4], [0.0])
    # std_min is inclusive: sd == std_min keeps the row, the next float above switches it off
    keep, _ = R.obs_norm_ref(tot, N, 2.0)
    drop, _ = R.obs_norm_ref(tot, N, np.nextafter(2.0, 3.0))
    assert sd[1] == 2.0 and keep[1] == 0.5 and drop[1] == 0.0
    assert _same(keep, [0.0, 0.5, 0.0, 1e-3, 0.0])
    # the variance is clamped: totals whose E[x^2] - mean^2 comes out below zero give +0.0, never the NaN of its square root
    total = np.r_[[3.0] + [0.0] * 4, [2.9999999999999996] + [0.0] * 4]
    assert 2.9999999999999996 / 3 - (3.0 / 3) * (3.0 / 3) < 0
    m, v = R.obs_moments_ref(total, 3)
    assert _same(v, np.zeros(5)) and m[0] == 1.0
    sc, sh = R.obs_norm_ref(total, 3, 1e-6)
    assert _same(sc, np.zeros(5)) and _same(sh, np.zeros(5))
    # a row that is constant up to rounding (1000 times 0.1: a variance of 1e-18 or so) is switched off by std_min, not blown up
    x = np.full(1000, 0.1)
    t = np.zeros(10)
    t[0], t[5] = np.sum(x), np.sum(x * x)
    m, v = R.obs_moments_ref(t, 1000)
    assert 0.0 <= v[0] < 1e-16
    sc, sh = R.obs_norm_ref(t, 1000, 1e-6)
    assert _same(sc, np.zeros(5)) and np.isfinite(sh).all()
    # against exact arithmetic: mean and variance of the four live rows within a few roundings of their own operations
    for k in range(4):
        xs = [Fraction(float(v)) for v in rows[k]]
        em = sum(xs) / N
        ev = sum(x * x for x in xs) / N - em * em
        assert Fraction(float(mean[k])) == em and Fraction(float(var[k])) == ev          # (these inputs are exact in binary)
    # the count converts as (double)uint64 does
    m, _ = R.obs_moments_ref(np.r_[[2.0 ** 60] * 5, [0.0] * 5], 2 ** 60 + 1)
    assert _same(m, np.ones(5))
