"""The cases tests/test_pg_log_host.py and tests/test_gpu_pg_log.py hold the training log of the policy-gradient loop to
(bsk_pg_episodes, bsk_pg_log_update; csrc/bsk_pglog.hip).  TEST CODE.

A case is the histories of one rollout, (T, n) each, and the state carried in.  Rewards are N(0.2, 1); a reason byte is non-zero at
``rate`` - a few ends per column at the sizes used - and then one of the four BSK_DONE bits; values are N(1, 1) in f32 and the
returns the values plus N(0, 0.5): var_y is about 1.25 at a mean of 1, of the order of mean_y**2, so that the bound on the
explained variance (tests/_pg_log_bounds.py) is some 1e-12 of a number of order 1."""
import numpy as np

SHAPES = [(n, T) for n in (1, 63, 64, 65, 300, 4097) for T in (1, 7, 9)]
HOST_SHAPES = [(1, 1), (1, 9), (63, 7), (65, 9), (300, 17)]
BITS = np.array([1, 2, 4, 8], np.uint8)


def episode_case(T, n, seed, rate=0.3, fresh=False):
    """-> dict: reward f64, reason u8, action i32, value f32, ret f64, each (T, n), and state = (ep_return f64 (n,), ep_len i32 (n,)),
    non-zero unless ``fresh``"""
    rng = np.random.default_rng(7000 + seed)
    reward = rng.normal(0.2, 1.0, (T, n))
    reason = np.where(rng.random((T, n)) < rate, BITS[rng.integers(0, 4, (T, n))], 0).astype(np.uint8)
    action = rng.integers(0, 3, (T, n)).astype(np.int32)
    value = rng.normal(1.0, 1.0, (T, n)).astype(np.float32)
    ret = value.astype(np.float64) + rng.normal(0.0, 0.5, (T, n))
    state = (np.zeros(n), np.zeros(n, np.int32)) if fresh else (rng.normal(0.0, 3.0, n), rng.integers(0, 500, n).astype(np.int32))
    return dict(reward=reward, reason=reason, action=action, value=value, ret=ret, state=state)


def padded(case, stride):
    """The histories as [T][stride] with what must never be read in the padding columns: NaN, reason 0xFF, action 1"""
    out = {}
    for k, fill in (("reward", np.nan), ("reason", 0xFF), ("action", 1), ("value", np.nan), ("ret", np.nan)):
        a = case[k]
        full = np.full((a.shape[0], stride), fill, a.dtype)
        full[:, :a.shape[1]] = a
        out[k] = full
    return out


def diag_case(n_rows, n_norms, seed, exact_one=True):
    """-> (diag f64 (n_rows, 8), norms f64 (n_norms, 2)): diagnostics rows of mixed sign and magnitude, and {norm, scale} rows of which
    about half are clipped (scale < 1), the first with a scale of exactly 1.0"""
    rng = np.random.default_rng(7500 + seed)
    diag = rng.normal(0.0, 1.0, (n_rows, 8)) * 10.0 ** rng.integers(-3, 4, (n_rows, 8))
    norm = rng.uniform(0.1, 1.0, n_norms)
    norms = np.stack([norm, 0.5 / np.maximum(norm, 0.5)], axis=1)
    if exact_one:
        norms[0] = (0.5, 1.0)
    return diag, norms
