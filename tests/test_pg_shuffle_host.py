"""CPU: what the shuffled minibatches and the clipped value loss of the policy-gradient loop state without a device - the
stateless permutation ``pg_perm_ref`` (include/bskgpu.h, bsk_pg_gather; csrc/bsk_shuffle.hpp), ``pg_gather_ref``,
``fit_value_delta_ref`` and the argument rules of ``check_pg_shuffle`` / ``check_pg_gather``.

The permutation is integer arithmetic: the numpy restatement and the device function are the same numbers.  The device function
itself, ``shuffle_perm`` with its uncapped cycle walk, is plain C++ and is compiled here for the HOST (tools/pg_perm_host.cpp) and
held to the restatement over every listed N, so that the bijection - and the walk's end - is shown before a GPU runs it.

The uniformity bound is derived, not measured: the chi-square of the N^2 = 10 000 cells (q, perm(q)) over 20 000 permutations that
are uniform has about (N - 1)^2 = 9 801 degrees of freedom, mean 9 801 and standard deviation sqrt(2 * 9 801) = 140; four standard
deviations above the mean, 10 361, is about its 1 - 3e-5 quantile.  The seed is fixed at 1 and was not searched for."""
import os
import subprocess

import numpy as np
import pytest

from basilisk_env_amd import policy as P

SIZES = (1, 2, 3, 5, 64, 65, 193, 4097, 12297, 65537)
STATES = ((0, 0), (1, 7), (2 ** 63 + 5, 2 ** 40 + 3), (2 ** 64 - 1, 2 ** 64 - 1))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the permutation
def test_the_round_keys_are_two_philox_draws_of_the_state_words():
    from basilisk_env_amd.policy_ref import philox4x32_10
    seed, epoch = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    k = P.pg_shuffle_keys_ref(seed, epoch)
    assert k.shape == (8,) and k.dtype == np.uint64 and (k < 2 ** 32).all()
    for i in range(2):
        w = philox4x32_10(epoch & 0xFFFFFFFF, epoch >> 32, 0x50475348, i, seed & 0xFFFFFFFF, seed >> 32)
        assert [int(x) for x in w] == [int(x) for x in k[4 * i:4 * i + 4]]
    many = P.pg_shuffle_keys_ref(seed, np.array([0, epoch, 5], np.uint64))
    assert many.shape == (8, 3) and np.array_equal(many[:, 1], k) and np.array_equal(many[:, 2], P.pg_shuffle_keys_ref(seed, 5))


@pytest.mark.parametrize("N", SIZES)
def test_the_permutation_is_a_bijection(N):
    q = np.arange(N)
    for seed, epoch in STATES:
        p = P.pg_perm_ref(seed, epoch, N, q)
        assert p.dtype == np.int64 and p.shape == (N,) and np.array_equal(np.sort(p), q), (N, seed, epoch)
        # a window is the window of the whole, whatever else is asked for beside it
        if N > 3:
            assert np.array_equal(P.pg_perm_ref(seed, epoch, N, q[1:N - 1].reshape(1, -1))[0], p[1:N - 1])


def test_epochs_and_seeds_give_different_permutations():
    N, q = 4097, np.arange(4097)
    base = P.pg_perm_ref(3, 0, N, q)
    for seed, epoch in ((3, 1), (3, 2), (4, 0), (3, 2 ** 32), (3 + 2 ** 32, 0)):
        other = P.pg_perm_ref(seed, epoch, N, q)
        # two independent uniform permutations agree in one place on average: far fewer than a tenth agree
        assert (other == base).sum() < N // 10, (seed, epoch)
    assert (base == q).sum() < N // 10


def test_the_permutation_refuses_what_lies_outside_its_domain():
    for N in (0, -1, 2 ** 31):
        with pytest.raises(ValueError):
            P.pg_perm_ref(0, 0, N, np.arange(1))
    for q in ([-1], [5]):
        with pytest.raises(ValueError):
            P.pg_perm_ref(0, 0, 5, np.array(q))
    with pytest.raises(ValueError):
        P.pg_perm_keys_ref(np.zeros((8, 3), np.uint64), 5, np.zeros((2, 5), np.int64))
    assert np.array_equal(P.pg_perm_ref(9, 9, 1, np.zeros(4, np.int64)), np.zeros(4, np.int64))


def test_pairs_of_position_and_image_are_uniform_over_the_epochs():
    N, E, seed = 100, 20000, 1
    q = np.broadcast_to(np.arange(N), (E, N))
    p = P.pg_perm_keys_ref(P.pg_shuffle_keys_ref(seed, np.arange(E)), N, q)
    assert np.array_equal(p[123], P.pg_perm_ref(seed, 123, N, np.arange(N)))       # (the vectorised path is the scalar one)
    counts = np.zeros((N, N), np.float64)
    np.add.at(counts, (q.ravel(), p.ravel()), 1.0)
    assert (counts.sum(axis=0) == E).all() and (counts.sum(axis=1) == E).all()
    chi2 = float((((counts - E / N) ** 2) / (E / N)).sum())
    bound = 9801 + 4 * np.sqrt(2 * 9801)
    print("chi-square of the (q, perm(q)) counts: %.1f on 9801 degrees of freedom, bound %.1f" % (chi2, bound))
    assert chi2 < bound, chi2


def test_the_device_function_compiled_for_the_host_is_the_restatement(tmp_path):
    """csrc/bsk_shuffle.hpp's shuffle_perm as the GPU will run it, walk and all, under the address and undefined-behaviour
    sanitizers of the host compiler: every listed N, every q."""
    exe = tmp_path / "pg_perm_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DBSK_SHUFFLE_HOST",
                           "-I", os.path.join(ROOT, "basilisk_env_amd", "csrc"), os.path.join(ROOT, "tools", "pg_perm_host.cpp"),
                           "-o", str(exe)])
    for N in SIZES:
        for seed, epoch in STATES[:3]:
            k = P.pg_shuffle_keys_ref(seed, epoch)
            out = subprocess.run([str(exe), str(N)] + [str(int(x)) for x in k], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stderr
            got = np.array(out.stdout.split(), np.int64)
            assert np.array_equal(got, P.pg_perm_keys_ref(k, N, np.arange(N))), (N, seed, epoch)


def test_gather_ref_is_a_take_by_the_permutation():
    T, n = 3, 7
    rng = np.random.default_rng(5)
    obs = rng.normal(size=(T, 5, n))
    action = rng.integers(0, 3, (T, n)).astype(np.int32)
    ret = rng.normal(size=(T, n))
    out = P.pg_gather_ref((2, 1), n, 4, 11, obs, action=action, ret=ret, value=None)
    s = P.pg_perm_ref(2, 1, T * n, 4 + np.arange(11))
    assert np.array_equal(out["index"], s) and set(out) == {"index", "obs", "action", "ret"}
    assert out["obs"].shape == (5, 11) and out["action"].dtype == np.int32
    for i, si in enumerate(s):
        assert np.array_equal(out["obs"][:, i], obs[si // n, :, si % n]) and out["action"][i] == action[si // n, si % n]
        assert out["ret"][i] == ret[si // n, si % n]
    ident = P.pg_gather_ref(None, n, n, n, obs, action=action)
    assert np.array_equal(ident["obs"], obs[1]) and np.array_equal(ident["action"], action[1])
    with pytest.raises(ValueError):
        P.pg_gather_ref(None, n, 15, 7, obs)


# ------------------------------------------------------------------------------------------------------------------ the value loss
F = np.float32


def _one(v, R, vo, cv, coef=0.5):
    d, t, c = P.fit_value_delta_ref(F([v]), np.array([R]), None if vo is None else F([vo]), cv, coef)
    assert d.dtype == np.float32 and t.dtype == np.float64 and c.dtype == bool
    return d[0], t[0], bool(c[0])


def _plain(v, R, coef=0.5):
    d = F(v) - F(R)
    return F(coef) * d, np.float64(d) * np.float64(d) * 0.5


def test_value_delta_without_old_values_is_the_squared_error():
    d, t, c = _one(1.25, -0.5, None, None)
    assert (d, t, c) == (*_plain(1.25, -0.5), False) and d == F(0.875) and t == 1.53125
    # the target is rounded to float32 first, as the kernel rounds it
    d, t, _ = _one(1.0, 1.0 + 2.0 ** -30, None, None)
    assert d == 0 and t == 0


def test_value_delta_inside_the_range_is_the_squared_error():
    assert _one(1.25, -0.5, 1.0, 0.5) == (*_plain(1.25, -0.5), False)
    assert _one(0.75, 3.0, 1.0, 0.5) == (*_plain(0.75, 3.0), False)


def test_value_delta_exactly_on_either_edge_is_inside():
    # dv = +-cv exactly: v = vo +- 0.5 in float32
    for v in (1.5, 0.5):
        for R in (-4.0, 4.0):
            assert _one(v, R, 1.0, 0.5) == (*_plain(v, R), False), (v, R)


def test_value_delta_outside_where_the_clipped_branch_holds_the_max_is_zero():
    # v moved from 1.0 up to 2.0 TOWARDS the target 3.0: clipped to 1.5, whose error 1.5 is the larger one
    d, t, c = _one(2.0, 3.0, 1.0, 0.5)
    assert c and d == 0 and not np.signbit(d) and t == 1.5 * 1.5 / 2
    # ... and down towards a target below
    d, t, c = _one(-1.0, -3.0, 1.0, 0.5)
    assert c and d == 0 and not np.signbit(d) and t == (0.5 + 3.0) ** 2 / 2


def test_value_delta_outside_where_the_unclipped_branch_holds_the_max_is_the_squared_error():
    # v moved from 1.0 up to 2.0 AWAY from the target 0.0: the unclipped error 2.0 is the larger one
    assert _one(2.0, 0.0, 1.0, 0.5) == (*_plain(2.0, 0.0), False)
    assert _one(-1.0, 2.0, 1.0, 0.5) == (*_plain(-1.0, 2.0), False)


def test_value_delta_a_tie_is_the_unclipped_branch():
    # v = 2.0, clipped to 1.5, target 1.75: both errors are 0.25
    d, t, c = _one(2.0, 1.75, 1.0, 0.5)
    assert not c and (d, t) == _plain(2.0, 1.75) and d == F(0.125)


def test_value_delta_takes_arrays_and_a_nan_difference_goes_outside_on_the_lower_side():
    v, R, vo = F([2.0, 2.0, 1.25, np.nan]), np.array([3.0, 0.0, -0.5, 0.0]), F([1.0, 1.0, 1.0, 1.0])
    d, t, c = P.fit_value_delta_ref(v, R, vo, 0.5, 1.0)
    assert list(c[:3]) == [True, False, False] and d[0] == 0 and d[1] == 2 and d[2] == F(1.75)
    assert not c[3] and np.isnan(d[3])              # (NaN > anything is false: the unclipped branch, which carries the NaN)


# ------------------------------------------------------------------------------------------------------------------ the rules
def test_the_loop_rules_of_shuffle_and_cliprange_vf():
    assert P.check_pg_shuffle() == (False, 0, None)
    assert P.check_pg_shuffle(True, 2 ** 64 - 1, 0.2, 8, 4, 1000) == (True, 2 ** 64 - 1, 0.2)
    assert P.check_pg_shuffle(np.bool_(True), np.int64(3), 1) == (True, 3, 1.0)
    for bad in (dict(shuffle=1), dict(shuffle=None), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.0), dict(seed=True),
                dict(cliprange_vf=0.0), dict(cliprange_vf=-0.2), dict(cliprange_vf=float("nan")), dict(cliprange_vf=float("inf")),
                dict(cliprange_vf=True), dict(n_envs=0), dict(n_steps=0), dict(minibatches=1.5),
                dict(shuffle=True, n_steps=2 ** 16, n_envs=2 ** 15)):
        with pytest.raises(ValueError):
            P.check_pg_shuffle(**bad)
    # the bound is the gather's: without shuffle nothing is gathered
    assert P.check_pg_shuffle(False, 0, None, 2 ** 16, 1, 2 ** 15) == (False, 0, None)
    assert P.check_pg_shuffle(True, 0, None, 2 ** 16 - 1, 1, 2 ** 15)[0]
    # check_pg_loop stays what it was
    assert P.check_pg_loop(8, 0.99, 0.95, 0.2, 0.01, 4, 4, 1) == (8, 0.99, 0.95, 0.2, 0.01, 4, 4, 1)


def test_the_gather_rules():
    assert P.check_pg_gather(4, 64, 64, 0, 256, 256) == (4, 64, 64, 0, 256, 256)
    assert P.check_pg_gather(2, 70, 96, 37, 101, 0) == (2, 70, 96, 37, 101, 0)
    for bad in ((0, 64, 64, 0, 1, 1), (4, 0, 64, 0, 1, 1), (4, 64, 63, 0, 1, 1), (4, 64, 64, -1, 1, 1), (4, 64, 64, 0, 0, 1),
                (4, 64, 64, 1, 256, 256), (4, 64, 64, 256, 1, 1), (2 ** 16, 2 ** 15, 2 ** 15, 0, 1, 1), (4, 64, 64, 0, 1.0, 1),
                (True, 64, 64, 0, 1, 1)):
        with pytest.raises(ValueError):
            P.check_pg_gather(*bad)
