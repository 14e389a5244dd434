"""Shapes and placements that take the column walks of the policy-gradient loop past their first trips - bsk_gae, bsk_reward_norm,
bsk_pg_episodes / bsk_pg_log_update and the lap shapes of bsk_adv_normalize (csrc/bsk_fit.hip: gae_kernel, adv_*_kernel;
csrc/bsk_rewnorm.hip; csrc/bsk_pglog.hip) -, shared by tests/test_gpu_pg_walks.py and its CPU twin
tests/test_pg_walk_cases_host.py.  TEST CODE.

Every kernel here walks [T][stride] histories one env per lane, joins per-wave partial rows and applies something elementwise.
``WHAT`` says what each shape is for; a failure message carries it (``tag``).
  row shapes    REWARD_NORM_BATCH = PG_EP_BATCH = 8 rows are in flight at once: T = 8 is one full batch and no tail, 16 the second
                trip of the batched loop - t is no longer 0 and the eight row registers are reused -, 17 that and a tail, 24 a third.
  grid shapes   reward_norm_apply_kernel's grid has min(T, 1024) rows and a block strides over the rest: T = 1024 is the last T
                without a second trip, 1025 the first with one (row 0's threads alone), 2049 gives row 0's threads three.
  lap shapes    a join has lane l add the partial rows l, l + 64, ...: 4096 envs are 64 waves - one entry in every lane, none
                empty -, 8192 are 128 - two in every lane -, 8321 are 131 - lanes 0 .. 2 take three, the rest two - and the last
                wave holds ONE env.
  GAE shapes    gae_kernel's loop is unrolled by four: T = 4 and 8 are whole unrolled trips, 5 and 9 leave a remainder of one, 33
                is eight trips and a remainder; 255, 256, 257 and 513 envs lie around the edges of workgroups of 256.
The cases themselves are the drawn ones of tests/_reward_norm_cases.py and tests/_pg_log_cases.py under their rule for the seed
(10 n + T); the reason bytes of the GAE cases are CONSTRUCTED, column c by ``GAE_KINDS[c % 7]``, over tests/test_pg_host.py's
drawn rewards and values."""
import numpy as np

from _pg_log_cases import episode_case
from _reward_norm_cases import reward_case, padded as reward_padded   # noqa: F401  (for tests/test_gpu_pg_walks.py)
from test_pg_host import gae_case

ROW_SHAPES = [(65, 8), (65, 16), (65, 17), (65, 24)]
GRID_SHAPES = [(1, 1024), (70, 1025), (3, 2049)]
LAP_SHAPES = [(4096, 9), (8192, 9), (8321, 9)]
WHAT = {(65, 8): "one full batch of rows, no tail", (65, 16): "two batches", (65, 17): "two batches and a tail", (65, 24): "three batches",
        (1, 1024): "the last T without a row stride", (70, 1025): "the first T with a row stride",
        (3, 2049): "row 0's threads take three trips",
        (4096, 9): "64 waves: one entry in every lane of the join", (8192, 9): "128 waves: two entries in every lane",
        (8321, 9): "131 waves: lanes 0 .. 2 take three entries, the rest two; a tail wave of one env"}
SEQUENCE_N, SEQUENCE_T = 65, (9, 16, 1)        # three calls on one state: a tail behind a batch, two batches, a tail alone
STALE_N = (300, 65)                            # a work buffer that a call at 300 envs has filled, then a call at 65 on it
LOG_UPDATE_ROWS, LOG_UPDATE_NORMS = (64, 65, 1000), (1, 65, None)

GAE_T, GAE_N = (4, 5, 8, 9, 33), (255, 256, 257, 513)
GAE_COEFS = [(0.97, 0.9), (0.0, 0.0), (1.0, 1.0)]
GAE_KINDS = ("last", "first", "every", "never", "first_and_last", "middle", "odd_rows")

# the loop off its one shape: a partial last wave, two batches of rows and a tail of two, three minibatches of six rows, a ring of
# two rows under three iterations
LOOP = dict(n_envs=200, n_steps=18, minibatches=3, epochs=2, hidden=(32, 16), value_hidden=(48,), max_grad_norm=0.5,
            cliprange_vf=0.2, log_capacity=2, iterations=3, max_length=5, gamma=0.97, lam=0.9, reward_clip=2.0, reward_eps=1e-8)


def tag(n, T):
    return "(n, T) = (%d, %d): %s" % (n, T, WHAT.get((n, T), "GAE shape"))


def waves(n):
    return (n + 63) // 64


def walk_reward_case(n, T, **kw):
    return reward_case(T, n, 10 * n + T, **kw)


def walk_episode_case(n, T, **kw):
    return episode_case(T, n, 10 * n + T, **kw)


def last_wave_case():
    """(8321, 9) with every reason byte zero but three of the LAST env's - the one env of wave 130: the extremes, the sums of the
    returns and every count of ended episodes come from that wave's partial row alone; the other 130 rows bring NaN and zeros"""
    n, T = LAP_SHAPES[-1]
    case = walk_episode_case(n, T)
    case["reason"][:] = 0
    case["reason"][[2, 5, 8], n - 1] = (1, 4, 8)
    return case


def sequence_cases(kind):
    """the three calls of different T on one state: ``kind`` "reward" or "episode" -> a list of cases; the first one's state and
    running values are what is carried in"""
    make = walk_reward_case if kind == "reward" else walk_episode_case
    return [make(SEQUENCE_N, T) for T in SEQUENCE_T]


def _tree(x):
    """the 64-lane tree over the last axis (..., W, 64) -> (..., W): lane l takes lane l + stride, stride 32 .. 1"""
    x = np.array(x, dtype=np.float64)
    for stride in (32, 16, 8, 4, 2, 1):
        x[..., :stride] = x[..., :stride] + x[..., stride:2 * stride]
    return x[..., 0]


def _pick_tree(x, greatest):
    x = np.array(x, dtype=np.float64)
    for stride in (32, 16, 8, 4, 2, 1):
        m, c = x[..., :stride], x[..., stride:2 * stride]
        with np.errstate(invalid="ignore"):
            x[..., :stride] = np.where(((c > m) if greatest else (c < m)) | np.isnan(m), c, m)
    return x[..., 0]


def episode_work_ref(case, keys=("reward", "reason", "action", "value", "ret")):
    """the partial rows bsk_pg_episodes leaves in its work buffer -> uint64 (W, 19): ``pg_episodes_walk_ref``'s per-lane values
    (lanes at and above n bring +0.0, NaN and 0) through the trees - seven sums, the two extremes, ten counts as integers"""
    from basilisk_env_amd import policy as P
    s, mn, mx, k, _ = P.pg_episodes_walk_ref(**{key: case[key] for key in tuple(keys) + ("state",)})
    n = s.shape[1]
    W = waves(n)
    lanes = np.zeros((7, W * 64), np.float64)
    lanes[:, :n] = s
    ext = np.full((2, W * 64), np.nan, np.float64)
    ext[0, :n], ext[1, :n] = mn, mx
    counts = np.zeros((10, W * 64), np.int64)
    counts[:, :n] = k
    out = np.empty((W, 19), np.uint64)
    with np.errstate(invalid="ignore", over="ignore"):
        out[:, :7] = _tree(lanes.reshape(7, W, 64)).T.copy().view(np.uint64)
    out[:, 7] = _pick_tree(ext[0].reshape(W, 64), False).view(np.uint64)
    out[:, 8] = _pick_tree(ext[1].reshape(W, 64), True).view(np.uint64)
    out[:, 9:] = counts.reshape(10, W, 64).sum(axis=2).T.astype(np.uint64)
    return out


# ------------------------------------------------------------------------------------------------------------------ bsk_gae
def gae_kind(c):
    return GAE_KINDS[c % len(GAE_KINDS)]


def gae_placement(T, n):
    """-> (reward f64 (T, n), reason u8 (T, n), value f32 (T, n), last_value f32 (n,)): tests/test_pg_host.py's drawn numbers under
    reason bytes placed by hand - column c ends an episode on its last row, on row 0, on every row, never, on row 0 and the last, on
    row T // 2, or on every odd row, by ``gae_kind(c)``; the byte is one of the four BSK_DONE bits in turn"""
    reward, _, value, last = gae_case(T, n, seed=100 * T + n)
    reason = np.zeros((T, n), np.uint8)
    for c in range(n):
        kind, bit = gae_kind(c), np.uint8(1 << (c % 4))
        if kind in ("last", "first_and_last"):
            reason[T - 1, c] = bit
        if kind in ("first", "first_and_last"):
            reason[0, c] = bit
        if kind == "every":
            reason[:, c] = bit
        if kind == "middle":
            reason[T // 2, c] = bit
        if kind == "odd_rows":
            reason[1::2, c] = bit
    return reward, reason, value, last


def gae_reach(reason):
    """-> bool (T, n): the samples ``last_value`` can reach - the rows behind a column's last end, every row of a column that has
    none.  The cut: with an end on the last row a column's estimates are the same with and without ``last_value``."""
    T, n = reason.shape
    ended = reason != 0
    last_end = np.where(ended.any(axis=0), T - 1 - np.argmax(ended[::-1], axis=0), -1)
    return np.arange(T)[:, None] > last_end[None, :]


POISON = (np.nan, np.inf, -np.inf)


def gae_poisoned(reward, value):
    """-> (reward, value, columns): copies with ONE column of every wave spoilt - a NaN, +inf or -inf in turn, in the reward of an
    even wave and in the value of an odd one, on row T // 2 - the lane moving from wave to wave (and into the one-lane tail wave)"""
    T, n = reward.shape
    reward, value = reward.copy(), value.copy()
    cols = []
    for w in range(waves(n)):
        c = min(64 * w + (11 * w + 3) % 64, n - 1)
        (reward if w % 2 == 0 else value)[T // 2, c] = POISON[w % 3]
        cols.append(c)
    return reward, value, np.array(cols)
