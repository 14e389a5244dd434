"""What tests/test_pg_sched_host.py and tests/test_gpu_pg_sched.py share: the cases of the schedule's rule and of the KL gate
(include/bskgpu.h: bsk_fit_set_schedule, bsk_fit_kl_gate), each with what the definition says of it written beside it.  TEST CODE.

INEXACT_PAIR is a pair whose a + (b - a) is NOT b in f64 - found by trying PPO2's usual ends on the CPU -, which is why the rule
returns b itself from ``total`` on: test_pg_sched_host.py asserts that it is such a pair."""
import numpy as np

INEXACT_PAIR = (0.2, 0.05)                 # clip annealed to a quarter: 0.2 + (0.05 - 0.2) = 0.05000000000000002
LR, CLIP, CLIP_VF, ENT = (1e-2, 0.0), INEXACT_PAIR, (0.3, 0.9), (0.01, 0.001)          # the four pairs the GPU tests anneal (b > a: clip_vf)

# (it, total, a, b, what the rule gives: "a", "b" or "line")
SCHEDULE_CASES = (
    (0, 4, 2.5e-4, 0.0, "a"), (0, 0, 2.5e-4, 0.0, "a"), (7, 0, 2.5e-4, 0.0, "a"), (2 ** 40, 0, 0.2, 0.05, "a"),          # it = 0, total = 0
    (4, 4, 2.5e-4, 0.0, "b"), (5, 4, 0.2, 0.05, "b"), (2 ** 63, 4, 0.2, 0.05, "b"), (4, 4) + INEXACT_PAIR + ("b",),      # it >= total
    (1, 1, 0.3, 0.9, "b"), (0, 1, 0.3, 0.9, "a"), (2, 1, 0.3, 0.9, "b"),                                              # total = 1
    (1, 4, 2.5e-4, 0.0, "line"), (3, 4, 0.2, 0.05, "line"), (1, 3, 0.3, 0.9, "line"), (2, 3, 0.3, 0.9, "line"),       # b > a among them
    (1, 3, 0.01, 0.001, "line"), (999, 1000, 1e-3, 1e-5, "line"), (1, 2, 0.2, 0.2, "line"),
    (2 ** 31 - 1, 2 ** 31, 2.5e-4, 0.0, "line"), (2 ** 31 - 1, 2 ** 31, 0.2, 0.05, "line"),                            # it = total - 1 at 2^31
    (2 ** 53 - 2, 2 ** 53 - 1, 0.3, 0.9, "line"), (1, 2 ** 53 - 1, 0.3, 0.9, "line"),
)


def gate_rows(kl_sums, counts, seed=0):
    """rows (n, 8) in the loop's ``log`` layout: column 0 the KL sums, column 7 the counts, the other six noise the gate must not read"""
    rng = np.random.default_rng(9100 + seed)
    rows = rng.normal(size=(len(kl_sums), 8))
    rows[:, 0], rows[:, 7] = kl_sums, counts
    return rows


def _mean(rows):
    S, N = rows[0, 0], rows[0, 7]
    for r in range(1, rows.shape[0]):
        S, N = S + rows[r, 0], N + rows[r, 7]
    return S / N


_THREE = gate_rows([0.75, 1.5, -0.25], [60.0, 64.0, 4.0], 1)              # mean 2 / 128 = 0.015625, exactly
MEAN = 0.015625

# (name, rows, kl_stop, gate in, skipped in, kl_at in) -> (gate, skipped, kl_at: None = the one that came in)
GATE_CASES = (
    ("mean exactly kl_stop: open", _THREE, MEAN, 0, 0, 0.0, (0, 0, None)),
    ("kl_stop just below the mean: closes", _THREE, np.nextafter(MEAN, 0.0), 0, 0, 0.0, (1, 1, MEAN)),
    ("mean just above kl_stop: closes", gate_rows([np.nextafter(2.0, 3.0)], [128.0], 2), MEAN, 0, 2, 0.0, (1, 3, np.nextafter(2.0, 3.0) / 128.0)),
    ("a NaN row closes", gate_rows([0.1, np.nan, 0.1], [64.0, 64.0, 2.0], 3), 0.5, 0, 0, 0.0, (1, 1, np.nan)),
    ("N = 0: open, whatever 0 / 0 is", gate_rows([0.0, 0.0], [0.0, 0.0], 4), 0.01, 0, 0, 0.0, (0, 0, None)),
    ("N = 0 with a sum: open", gate_rows([5.0], [0.0], 5), 0.01, 0, 0, 0.0, (0, 0, None)),
    ("already closed: stays closed, counts on, keeps the KL", gate_rows([0.0, 0.0], [64.0, 64.0], 6), 0.5, 1, 3, 0.75, (1, 4, None)),
    ("already closed and above again: the first KL stays", _THREE, 0.001, 1, 1, 0.75, (1, 2, None)),
    ("a negative mean: open", gate_rows([-3.0, 1.0], [64.0, 64.0], 7), 1e-9, 0, 0, 0.0, (0, 0, None)),
    ("nine rows", gate_rows(np.linspace(0.1, 0.9, 9), np.full(9, 64.0), 8), 0.007, 0, 0, 0.0, (1, 1, None)),
)


def gate_want(case):
    """the expectation of a GATE_CASES entry with its None filled in -> (gate, skipped, kl_at)"""
    name, rows, stop, gate, skipped, at, (g, k, a) = case
    if a is None:
        a = _mean(rows) if (g == 1 and gate == 0) else at
    return g, k, np.float64(a)
