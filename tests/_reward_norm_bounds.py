"""Error bound of the standard deviation behind the reward scaling of the policy-gradient loop (csrc/bsk_rewnorm.hip; definition in
include/bskgpu.h, bsk_reward_norm) against a plain per-env Python loop and numpy.var in f64 - derived, not tuned, in the calculus
of tests/_pg_log_bounds.py: u = 2**-53, g(k) the bound on the relative error of a sum of k + 1 terms in any order, FP64_SLACK for
the arithmetic of the bound itself.  TEST CODE.

What is exact.  The running return R of an env is one chain gamma * R + reward in a fixed order, which the plain loop repeats
operation for operation: the returns are the SAME f64 numbers on both sides, and so are their squares (one rounding each).  The
sums differ in ORDER only - the carried sum, the lanes' chains, the trees and the final addition are one summation tree over all
the terms - which ``_pg_log_bounds.sum_bound`` covers.

The deviation (``sd_bound``).  For N returns of magnitude at most M, ``_pg_log_bounds.var_bound`` gives
  |var^ - numpy.var| <= E_var,  var^ = max(S2 / N - (S1 / N)**2, 0)
  a^ = fl(var^ + eps) against b = fl(numpy.var + eps), one addition rounded on either side:
      |a^ - b| <= D = E_var + u (2 (numpy.var + eps) + E_var)
  |sqrt(a^) - sqrt(b)| = |a^ - b| / (sqrt(a^) + sqrt(b)) <= D / sqrt(b)        (b > 0 is asserted)
  one square root rounded on either side:  + u (2 sqrt(b) + D / sqrt(b))
"""
import numpy as np

from _pg_cond_bounds import U64
from _pg_log_bounds import var_bound
from _policy_bounds import FP64_SLACK


def sd_bound(returns, eps):
    """-> the bound on |restatement's sd - sqrt(numpy.var(returns) + eps)|; ``returns``: every return the statistics hold, as both
    sides form them"""
    x = np.asarray(returns, np.float64).reshape(-1)
    E_var = var_bound(x.size, np.abs(x).max())
    b = float(np.var(x)) + float(eps)
    assert b > 0.0
    D = E_var + U64 * (2.0 * b + E_var)
    root = np.sqrt(b)
    return (D / root + U64 * (2.0 * root + D / root)) * FP64_SLACK
