"""Error bounds of the training-log row of the policy-gradient loop (csrc/bsk_pglog.hip; definition in include/bskgpu.h,
bsk_pg_episodes) against a plain per-env Python loop and numpy.sum / numpy.var in f64 - derived, not tuned, in the calculus of
tests/_pg_cond_bounds.py: u = 2**-53, g(k) = k u / (1 - k u) the bound on the relative error of a sum of k + 1 terms IN ANY ORDER (so
the fixed order of the device and numpy's pairwise one are both covered), FP64_SLACK for the arithmetic of the bound itself.  TEST
CODE.

What is exact.  The running return R of an env is one chain of additions in a fixed order, which the plain loop repeats operation for
operation: the returns of the ended episodes are the SAME f64 numbers on both sides.  So the counts, the lengths and the two
extremes are equal, not close; so is every term of a sum - R * R, e = ret - (double)value and e * e carry one rounding each, the
same one on both sides.  Only the ORDER of the sums differs.

The sums (``sum_bound``).  A sum of k terms x_i that are the same on both sides, each side within g(k - 1) sum |x_i| of the true
sum:  |restatement - numpy.sum| <= 2 g(k - 1) sum |x_i|.

The explained variance (``explained_variance_bound``).  For N samples x_i of magnitude at most M, as in _pg_cond_bounds.py:
  mean = S1 / N                            e_mean = (g(N) + 2 u) M
  e2 = S2 / N, x * x rounded once:         e_e2 = (g(N) + 3 u) M**2
  var = e2 - mean * mean:                  e_var = e_e2 + (2 M e_mean + e_mean**2) + u (M + e_mean)**2 + 2 u M**2
                                           (the clamp at zero moves the computed value towards the true one)
  numpy.var, the mean of squared deviations, each below (2 M)**2 and formed with three roundings:  g(N + 4) 4 M**2
  E_var = e_var + g(N + 4) 4 M**2
With ratio = var_e / var_y and both variances off by E_e and E_y (var_y - E_y > 0 is asserted by the caller's choice of inputs:
var_y of the order of mean_y**2, so that E_y is some 1e-12 of it):
  |ratio^ - ratio| <= (E_e + ratio E_y) / (var_y - E_y), one division rounded on either side:  + 2 u ratio
  ev = 1 - ratio, one subtraction rounded on either side:  + 2 u (1 + ratio)
"""
import numpy as np

from _pg_cond_bounds import U64, g
from _policy_bounds import FP64_SLACK


def sum_bound(terms):
    """-> the bound on |restatement - numpy.sum(terms)| for terms that are the same numbers on both sides"""
    terms = np.asarray(terms, np.float64).reshape(-1)
    if terms.size < 2:
        return 0.0
    return 2.0 * g(terms.size - 1) * float(np.abs(terms).sum()) * FP64_SLACK


def var_bound(N, M):
    """-> E_var: the bound on |max(S2 / N - (S1 / N)**2, 0) - numpy.var| for N samples of magnitude at most M"""
    N, M = int(N), float(M)
    e_mean = (g(N) + 2.0 * U64) * M
    e_var = (g(N) + 3.0 * U64) * M * M + (2.0 * M * e_mean + e_mean ** 2) + U64 * (M + e_mean) ** 2 + 2.0 * U64 * M * M
    return e_var + g(N + 4) * 4.0 * M * M


def explained_variance_bound(y, e):
    """-> the bound on |restatement - (1 - numpy.var(e) / numpy.var(y))|; ``y`` the returns, ``e`` = y - value as both sides form it"""
    y, e = np.asarray(y, np.float64).reshape(-1), np.asarray(e, np.float64).reshape(-1)
    var_y, var_e = float(np.var(y)), float(np.var(e))
    E_y, E_e = var_bound(y.size, np.abs(y).max()), var_bound(e.size, np.abs(e).max())
    assert var_y - E_y > 0.0
    ratio = var_e / var_y
    return ((E_e + ratio * E_y) / (var_y - E_y) + 2.0 * U64 * ratio + 2.0 * U64 * (1.0 + ratio)) * FP64_SLACK
