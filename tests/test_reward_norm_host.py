"""CPU: what the reward scaling of the policy-gradient loop states without a device - ``reward_norm_ref`` (include/bskgpu.h,
bsk_reward_norm; csrc/bsk_rewnorm.hip), the argument rules ``check_reward_norm``, and the per-column walk of csrc/bsk_rewnorm.hpp
itself, compiled for the HOST (tools/reward_norm_host.cpp) under the address and undefined-behaviour sanitizers and held to the
restatement bit for bit, before a GPU runs it.

The restatement is held to a plain per-env Python loop with numpy.sum / numpy.var: the running returns and the count EQUAL - the
returns are the same f64 numbers on both sides -, the two sums within the bound of a reordered sum (tests/_pg_log_bounds.py) and
the deviation within the bound derived from it in tests/_reward_norm_bounds.py.  No case is skipped."""
import os
import subprocess

import numpy as np
import pytest

from _device_bits import same as _same
from _pg_log_bounds import sum_bound
from _reward_norm_bounds import sd_bound
from _reward_norm_cases import CLIP, EPS, GAMMA, HOST_SHAPES, PRIOR, SHAPES, reward_case, state_words
from basilisk_env_amd import _lib
from basilisk_env_amd import policy as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = {name: c for c, name in enumerate(P.REWARD_NORM_STATE_FIELDS)}


def _f(words):
    return words.view(np.float64)


def _plain(case, gamma):
    """one env after the other, one row after the other -> (every return counted, in the walk's order per env, new ret_run)"""
    T, n = case["reward"].shape
    g = float(gamma)
    returns, R_out = [], np.empty(n, np.float64)
    for j in range(n):
        R = float(case["ret_run"][j])
        for t in range(T):
            R = g * R + float(case["reward"][t, j])
            returns.append(R)
            if case["reason"][t, j]:
                R = 0.0
        R_out[j] = R
    return np.array(returns, np.float64), R_out


def _ref(case, gamma=GAMMA, eps=EPS, clip=CLIP, update=1, **kw):
    return P.reward_norm_ref(case["reward"], case["reason"], gamma, eps, clip, update, case["state"], case["ret_run"], **kw)


def test_the_state_words_are_named_once():
    assert P.REWARD_NORM_STATE_WORDS == 8 == len(P.REWARD_NORM_STATE_FIELDS) == len(set(P.REWARD_NORM_STATE_FIELDS))
    assert F["count"] == 2 and F["sd"] == 5 and F["calls"] == 6
    fresh = P.reward_norm_state_words(None)
    assert fresh.dtype == np.uint64 and fresh.shape == (8,) and not fresh.any() and P.reward_norm_divisor(fresh) == 1.0
    for bad in (np.zeros(8), np.zeros(7, np.uint64)):
        with pytest.raises(ValueError):
            P.reward_norm_state_words(bad)


def test_every_case_used_has_a_positive_variance_and_none_is_skipped():
    shapes = sorted(set(SHAPES) | set(HOST_SHAPES))
    assert len(shapes) == len(SHAPES) + len(HOST_SHAPES) - 4       # all but (300, 17) are in both
    for n, T in shapes:
        case = reward_case(T, n, 10 * n + T)
        out, words, R = _ref(case)
        assert _f(words)[F["var"]] > 0.0 and _f(case["state"])[F["var"]] > 0.0, (n, T)
        assert (case["ret_run"] != 0).all() and case["state"][:3].all() and case["prior"].size == PRIOR
        assert (np.abs(out) == CLIP).any() or T * n < 16, (n, T)     # the clip is met in all but the smallest cases
        assert (np.abs(out) < CLIP).any() or T * n < 16, (n, T)


@pytest.mark.parametrize("n,T", HOST_SHAPES)
def test_the_restatement_against_a_plain_loop(n, T):
    case = reward_case(T, n, 10 * n + T)
    out, words, R = _ref(case)
    assert out.shape == (T, n) and out.dtype == np.float64 and words.dtype == np.uint64 and R.dtype == np.float64
    returns, want_R = _plain(case, GAMMA)
    assert _same(R, want_R)
    assert int(words[F["count"]]) == PRIOR + T * n and int(words[F["calls"]]) == 4 and int(words[F["zero"]]) == 0
    everything = np.r_[case["prior"], returns]
    for c, terms in ((F["sum"], everything), (F["sum_sq"], everything * everything)):
        bound = sum_bound(terms)
        print("word %d: |difference| %.3e, bound %.3e" % (c, abs(_f(words)[c] - terms.sum()), bound))
        assert abs(_f(words)[c] - terms.sum()) <= bound, c
    want_sd = np.sqrt(np.var(everything) + EPS)
    bound = sd_bound(everything, EPS)
    print("sd %.6f: |difference| %.3e, bound %.3e" % (want_sd, abs(_f(words)[F["sd"]] - want_sd), bound))
    assert bound < 1e-9 and abs(_f(words)[F["sd"]] - want_sd) <= bound
    # the words that follow from the three sums, and the rollout scaled by the deviation that already holds it
    mean = _f(words)[F["sum"]] / np.float64(PRIOR + T * n)
    var = _f(words)[F["sum_sq"]] / np.float64(PRIOR + T * n) - mean * mean
    assert _same(_f(words)[[F["mean"], F["var"], F["sd"]]], np.array([mean, var, np.sqrt(var + np.float64(EPS))]))
    assert _same(out, np.clip(case["reward"] / _f(words)[F["sd"]], -CLIP, CLIP))
    assert not _same(case["state"], words)                     # (the state that came in is not changed in place)


def test_two_rollouts_with_carried_state_are_the_one_they_make():
    whole = reward_case(6, 70, 3)
    first = dict(whole, reward=whole["reward"][:3], reason=whole["reason"][:3])
    _, words, R = _ref(first)
    second = dict(whole, reward=whole["reward"][3:], reason=whole["reason"][3:], state=words, ret_run=R)
    _, words, R = _ref(second)
    _, want_words, want_R = _ref(whole)
    assert _same(R, want_R) and words[F["count"]] == want_words[F["count"]] == PRIOR + 6 * 70
    assert words[F["calls"]] == 5 and want_words[F["calls"]] == 4
    returns, _ = _plain(whole, GAMMA)
    everything = np.r_[whole["prior"], returns]
    assert abs(_f(words)[F["sum"]] - _f(want_words)[F["sum"]]) <= sum_bound(everything)


def test_the_branches_of_the_restatement():
    case = reward_case(5, 65, 4)
    # gamma = 0: the returns are the rewards
    a1, a2, k, R = P.reward_norm_walk_ref(case["reward"], case["reason"], 0.0, case["ret_run"])
    s1 = np.zeros(65)
    for t in range(5):
        s1 = s1 + case["reward"][t]
    assert _same(a1, s1) and (k == 5).all()
    assert _same(R, np.where(case["reason"][4] != 0, 0.0, case["reward"][4]))
    # every reason set: nothing is carried, and the zero is +0.0
    every = dict(case, reason=np.full_like(case["reason"], 4), reward=-np.abs(case["reward"]))
    _, words, R = _ref(every)
    assert _same(R, np.zeros(65)) and not np.signbit(R).any()
    # no reason set: one discounted chain per env
    quiet = dict(case, reason=np.zeros_like(case["reason"]))
    _, _, R = _ref(quiet)
    chain = case["ret_run"].copy()
    for t in range(5):
        chain = np.float64(GAMMA) * chain + case["reward"][t]
    assert _same(R, chain)
    # update = 0 on a fresh state: the identity under the clip, and nothing is carried
    fresh = reward_case(5, 65, 4, fresh=True)
    out, words, R = _ref(fresh, update=0)
    inside = np.abs(fresh["reward"]) <= CLIP
    assert inside.any() and not inside.all()
    assert _same(out[inside], fresh["reward"][inside]) and _same(out[~inside], np.copysign(CLIP, fresh["reward"][~inside]))
    assert not words.any() and not R.any()
    # update = 0 with a state: frozen, and None stands for the fresh one
    out, words, R = _ref(case, update=0)
    assert _same(words, case["state"]) and _same(R, case["ret_run"])
    assert _same(out, np.clip(case["reward"] / _f(case["state"])[F["sd"]], -CLIP, CLIP))
    assert _same(P.reward_norm_ref(fresh["reward"], fresh["reason"], GAMMA, EPS, CLIP, 1)[0], _ref(fresh)[0])
    # the partial rows
    out, words, R, work = _ref(case, with_work=True)
    assert work.shape == (2, 3) and work.dtype == np.uint64 and list(work[:, 2]) == [64 * 5, 5]
    assert _ref(case, update=0, with_work=True)[3] is None


def test_the_clip_edges_and_no_clip_and_a_nan():
    case = reward_case(3, 65, 5)
    sd = _f(case["state"])[F["sd"]]
    edge = CLIP * sd
    case["reward"][0, :8] = [edge * (1 + 2.0 ** -40), edge * (1 - 2.0 ** -40), -edge * (1 + 2.0 ** -40), -edge * (1 - 2.0 ** -40),
                             np.inf, -np.inf, np.nan, -0.0]
    out, _, _ = _ref(case, update=0)
    got = out[0, :8]
    assert got[0] == CLIP and got[2] == -CLIP and got[4] == CLIP and got[5] == -CLIP
    assert 0 < got[1] < CLIP and -CLIP < got[3] < 0 and _same(got[[1, 3]], case["reward"][0, [1, 3]] / sd)
    assert np.isnan(got[6]) and _same(got[7], np.float64(-0.0))
    wide, _, _ = _ref(case, update=0, clip=np.inf)
    assert _same(wide, case["reward"] / sd) and np.isinf(wide[0, 4:6]).all() and (np.abs(wide[1:]) > CLIP).any()


def test_scaling_everything_by_a_power_of_two_scales_the_deviation_and_nothing_else():
    """with eps = 0 the arithmetic is homogeneous: rewards, ret_run and sum times 4, sum_sq times 16 -> sd times 4 exactly, out the
    same bits"""
    case = reward_case(9, 130, 6)
    out, words, R = _ref(case, eps=0.0)
    big = dict(case, reward=case["reward"] * 4.0, ret_run=case["ret_run"] * 4.0, state=case["state"].copy())
    _f(big["state"])[[F["sum"], F["sum_sq"]]] = _f(case["state"])[[F["sum"], F["sum_sq"]]] * np.array([4.0, 16.0])
    out4, words4, R4 = _ref(big, eps=0.0)
    assert _same(out4, out) and _same(R4, R * 4.0)
    assert _same(_f(words4)[[F["sum"], F["sum_sq"], F["mean"], F["var"], F["sd"]]],
                 _f(words)[[F["sum"], F["sum_sq"], F["mean"], F["var"], F["sd"]]] * np.array([4.0, 16.0, 4.0, 16.0, 4.0]))
    assert words4[F["count"]] == words[F["count"]]


def test_the_argument_rules():
    assert P.check_reward_norm(8, 65, 70, 0.99, 1e-8, 10.0) == (8, 65, 70, 0.99, 1e-8, 10.0)
    assert P.check_reward_norm(2 ** 15, 2 ** 16, 2 ** 16, 0, 0, np.inf) == (2 ** 15, 2 ** 16, 2 ** 16, 0.0, 0.0, np.inf)
    assert P.check_reward_norm(1, 1, 1, 1.0, 0.0, 1e-300)[3] == 1.0
    for bad in ((0, 1, 1, 0.9, 0.0, 1.0), (1, 0, 1, 0.9, 0.0, 1.0), (1, 2, 1, 0.9, 0.0, 1.0), (2 ** 15, 2 ** 16, 2 ** 16 + 1, 0.9, 0.0, 1.0),
                (1.0, 1, 1, 0.9, 0.0, 1.0), (True, 1, 1, 0.9, 0.0, 1.0), (1, 1, 1, -0.1, 0.0, 1.0), (1, 1, 1, 1.1, 0.0, 1.0),
                (1, 1, 1, np.nan, 0.0, 1.0), (1, 1, 1, np.inf, 0.0, 1.0), (1, 1, 1, 0.9, -1e-9, 1.0), (1, 1, 1, 0.9, np.inf, 1.0),
                (1, 1, 1, 0.9, np.nan, 1.0), (1, 1, 1, 0.9, 0.0, 0.0), (1, 1, 1, 0.9, 0.0, -1.0), (1, 1, 1, 0.9, 0.0, np.nan),
                (1, 1, 1, 0.9, 0.0, -np.inf)):
        with pytest.raises(ValueError):
            P.check_reward_norm(*bad)
    for n in (1, 63, 64, 65, 4097, 65536):
        assert P.reward_norm_work_bytes(n) == 8 * 3 * ((n + 63) // 64)
    with pytest.raises(ValueError):
        P.reward_norm_work_bytes(0)
    case = reward_case(2, 3, 7)
    for bad in (dict(ret_run=np.zeros(2)), dict(state=np.zeros(8))):
        with pytest.raises(ValueError):
            _ref(dict(case, **bad))
    with pytest.raises(ValueError):
        P.reward_norm_ref(np.zeros(3), np.zeros(3), 0.9, 0.0, 1.0, 1)


def test_the_symbols_are_declared_and_exported():
    lib = _lib.load()
    for name in ("bsk_reward_norm_work_bytes", "bsk_reward_norm"):
        assert name in _lib.EXPORTS and name in _lib.SIGNATURES and hasattr(lib, name), name
    with open(os.path.join(ROOT, "include", "bskgpu.h")) as f:
        header = f.read()
    assert "int64_t bsk_reward_norm_work_bytes(int n);" in header and "#define BSK_REWARD_NORM_STATE_WORDS 8" in header
    assert "int bsk_reward_norm(const double* d_reward_hist, const uint8_t* d_reason_hist, int n_steps, int n_envs, int64_t stride," in header
    for n in (1, 64, 65, 65536):
        assert lib.bsk_reward_norm_work_bytes(n) == P.reward_norm_work_bytes(n)
    assert lib.bsk_reward_norm_work_bytes(0) == 0 and lib.bsk_reward_norm_work_bytes(-5) == 0
    # refused before anything is launched: no device is needed to be told so
    assert lib.bsk_reward_norm(None, None, 1, 1, 1, 0.99, 1e-8, 10.0, 1, None, None, None, None, None) == -1
    assert lib.bsk_reward_norm(None, None, 1, 1, 1, 0.99, 1e-8, 10.0, 0, None, None, None, None, None) == -1
    assert callable(P.reward_normalize)


def _hex64(a):
    return ["%016x" % int(b) for b in np.ascontiguousarray(a, np.float64).view(np.uint64).reshape(-1)]


def test_the_device_walk_compiled_for_the_host_is_the_restatement(tmp_path):
    """csrc/bsk_rewnorm.hpp's reward_norm_walk as the GPU will run it - batches of eight rows, the tail, strided columns - under the
    address and undefined-behaviour sanitizers of the host compiler: the two sums, the count and the new running return of every
    column equal what the restatement holds in front of the trees, in every bit."""
    exe = tmp_path / "reward_norm_host"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DBSK_REWNORM_HOST", "-I", os.path.join(ROOT, "basilisk_env_amd", "csrc"),
                           os.path.join(ROOT, "tools", "reward_norm_host.cpp"), "-o", str(exe)])
    for n, T in HOST_SHAPES:
        case = reward_case(T, n, 10 * n + T)
        for gamma in (GAMMA, 0.0, 1.0):
            lines = _hex64(np.float64(gamma)) + _hex64(case["ret_run"])
            lines += ["%s %d" % c for c in zip(_hex64(case["reward"]), case["reason"].reshape(-1))]
            out = subprocess.run([str(exe), str(T), str(n), str(n + 5)], input="\n".join(lines) + "\n", capture_output=True, text=True,
                                 timeout=120)
            assert out.returncode == 0, out.stderr
            got = [line.split() for line in out.stdout.splitlines()]
            assert len(got) == n and all(len(g) == 4 for g in got)
            a1, a2, k, R = P.reward_norm_walk_ref(case["reward"], case["reason"], gamma, case["ret_run"])
            f = np.array([[int(g[0], 16), int(g[1], 16), int(g[3], 16)] for g in got], np.uint64)
            want = np.ascontiguousarray(np.stack([a1, a2, R], axis=1)).view(np.uint64)
            assert np.array_equal(f, want), (n, T, gamma)
            assert np.array_equal(np.array([int(g[2]) for g in got], np.int64), k), (n, T, gamma)


def test_state_words_of_the_cases_are_what_the_restatement_would_leave():
    """the carried state of the cases is an honest one: a fresh state updated with the prior returns as one column of rewards under
    gamma = 0 has the same count and, within the reordered-sum bound, the same sums"""
    prior = reward_case(1, 1, 0)["prior"]
    _, words, _ = P.reward_norm_ref(prior[:, None], np.zeros((PRIOR, 1), np.uint8), 0.0, EPS, CLIP, 1)
    want = state_words(prior, calls=1)
    assert words[F["count"]] == want[F["count"]] == PRIOR and words[F["calls"]] == 1
    assert abs(_f(words)[F["sum"]] - _f(want)[F["sum"]]) <= sum_bound(prior)
    assert abs(_f(words)[F["sum_sq"]] - _f(want)[F["sum_sq"]]) <= sum_bound(prior * prior)
