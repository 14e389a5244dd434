"""The cases tests/test_reward_norm_host.py and tests/test_gpu_reward_norm.py hold the reward scaling of the policy-gradient loop to
(bsk_reward_norm; csrc/bsk_rewnorm.hip).  TEST CODE.

A case is the two histories of one rollout, (T, n) each, and what is carried in: every env's running discounted return, N(0, 3) and
so not zero, and the eight state words - the sums of ``PRIOR`` earlier returns drawn from N(0.5, 1.5), kept in the case so that a
plain loop can repeat the statistics over all of them; their variance is about 2.25 at a mean of 0.5, so var > 0 at every shape,
the single sample of (1, 1) included.  Rewards are N(0.2, 1); a reason byte is non-zero at ``rate`` and then one of the four
BSK_DONE bits."""
import numpy as np

SHAPES = [(n, T) for n in (1, 63, 64, 65, 300, 4097) for T in (1, 7, 9)]
HOST_SHAPES = [(1, 1), (1, 9), (63, 7), (65, 9), (300, 17)]
BITS = np.array([1, 2, 4, 8], np.uint8)
PRIOR = 200
GAMMA, EPS, CLIP = 0.97, 1e-8, 0.5          # a clip that a good part of N(0.2, 1) / sd exceeds on either side


def state_words(prior, calls=3, eps=EPS):
    """-> uint64 (8,): the state after ``calls`` updating calls that saw the returns ``prior`` (all zero for none)"""
    words = np.zeros(8, np.uint64)
    prior = np.asarray(prior, np.float64).reshape(-1)
    if prior.size:
        f = words.view(np.float64)
        f[0], f[1] = prior.sum(), (prior * prior).sum()
        mean = f[0] / prior.size
        var = max(f[1] / prior.size - mean * mean, 0.0)
        f[3], f[4], f[5] = mean, var, np.sqrt(var + eps)
        words[2], words[6] = prior.size, calls
    return words


def reward_case(T, n, seed, rate=0.3, fresh=False):
    """-> dict: reward f64 and reason u8, each (T, n); ret_run f64 (n,) and state u64 (8,), non-zero unless ``fresh``; prior f64: the
    returns behind the state"""
    rng = np.random.default_rng(9000 + seed)
    reward = rng.normal(0.2, 1.0, (T, n))
    reason = np.where(rng.random((T, n)) < rate, BITS[rng.integers(0, 4, (T, n))], 0).astype(np.uint8)
    ret_run = rng.normal(0.0, 3.0, n)
    prior = rng.normal(0.5, 1.5, PRIOR)
    if fresh:
        ret_run, prior = np.zeros(n), np.zeros(0)
    return dict(reward=reward, reason=reason, ret_run=ret_run, state=state_words(prior), prior=prior)


def padded(case, stride):
    """The histories as [T][stride] with what must never be read in the padding columns: NaN and reason 0xFF"""
    out = {}
    for k, fill in (("reward", np.nan), ("reason", 0xFF)):
        a = case[k]
        full = np.full((a.shape[0], stride), fill, a.dtype)
        full[:, :a.shape[1]] = a
        out[k] = full
    return out
