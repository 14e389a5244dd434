"""Error bounds of the two reductions that condition the policy-gradient update (csrc/bsk_fit.hip: adv_*_kernel, fit_gnorm_kernel;
definition in include/bskgpu.h, bsk_adv_normalize and bsk_fit_set_max_grad_norm) against plain numpy in f64 - derived, not tuned,
in the calculus of tests/_pg_bounds.py carried to f64: u = 2**-53, g(k) = k u / (1 - k u) the bound on the relative error of a sum of
k + 1 terms IN ANY ORDER (so the fixed order of the device and numpy's pairwise one are both covered), FP64_SLACK for the
arithmetic of the bound itself.  TEST CODE.

Advantage normalisation (``adv_moments_bound``, ``adv_out_bound``).  The N counting samples are f32 numbers widened exactly, of
magnitude at most M.
  S1              a sum of N exact terms:                       |S1^ - S1| <= g(N) N M
  mean = S1 / N   one division:                                 e_mean = (g(N) + 2 u) M
  S2              x * x is exact in f64, then a sum:            |S2^ - S2| <= g(N) N M**2;   e_e2 = (g(N) + 2 u) M**2
  var = e2 - mean * mean, one product and one subtraction, each rounded, of numbers below M**2 (1 + small):
                  e_var = e_e2 + (2 M e_mean + e_mean**2) + u (M + e_mean)**2 + 2 u M**2
                  (the clamp at zero moves the computed value towards the true one, which is not negative)
  numpy           mean: pairwise, e <= g(N) M + u M, inside e_mean once more;  var as the mean of squared deviations, each below
                  (2 M)**2 and formed with three roundings:  e <= g(N + 4) 4 M**2
  sd = sqrt(var)  |sqrt(a) - sqrt(b)| <= min(sqrt(|a - b|), |a - b| / sqrt(b)), one rounding on either side:
                  e_sd = min(sqrt(E_var), E_var / sd) + 2 u (sd + sqrt(E_var))
  out             d = x - mean:  e_d = E_mean + u (|d| + E_mean);   inv = 1 / (sd + eps), with a = sd^ + eps and b = sd + eps:
                  e_inv = e_sd / (a b) + 2 u / a;   the product:  e_d inv^ + |d| e_inv + u (|d| + e_d) inv^;   rounded to f32 on
                  both sides:  2 * (2**-24 |out| + 2**-150)

The gradient's norm (``grad_norm_rel_bound``).  g_q = A_q / count carries one rounding, its square one more on a number already
off by one: (1 + u)**3; the sum of n terms g(n - 1); the root halves the relative error and adds one rounding.  All of it below
g(n + 4); ``numpy.linalg.norm`` of the same quotients is within g(n + 2) of the truth on its side.  The norm AFTER the clip,
``numpy.linalg.norm((A / count) * scale)`` with scale = max_norm / norm^ (one rounding) and one rounding per product, is therefore
max_norm to within max_norm (g(n + 4) + 2 u + g(n + 2)).
"""
import numpy as np

from _policy_bounds import FP64_SLACK

U64 = 2.0 ** -53


def g(k):
    return k * U64 / (1.0 - k * U64)


def adv_moments_bound(N, M, sd):
    """-> (E_mean, E_sd): bounds on |restatement - numpy.mean| and |restatement - numpy.std| for N samples of magnitude at most M
    whose f64 standard deviation is ``sd``."""
    N, M, sd = int(N), float(M), float(sd)
    e_mean = (g(N) + 2.0 * U64) * M
    e_var = (g(N) + 2.0 * U64) * M * M + (2.0 * M * e_mean + e_mean ** 2) + U64 * (M + e_mean) ** 2 + 2.0 * U64 * M * M
    E_mean = (e_mean + g(N) * M + U64 * M) * FP64_SLACK
    E_var = e_var + g(N + 4) * 4.0 * M * M
    root = np.sqrt(E_var)
    e_sd = (min(root, E_var / sd) if sd > 0.0 else root) + 2.0 * U64 * (sd + root)
    return E_mean, e_sd * FP64_SLACK


def adv_out_bound(x, mean, sd, sd_hat, eps, E_mean, E_sd):
    """-> the bound on |restatement - float32((x - mean) / (sd + eps))| per sample, ``mean`` and ``sd`` numpy's, ``sd_hat`` the
    restatement's."""
    d = np.abs(np.asarray(x, np.float64) - mean)
    e_d = E_mean + U64 * (d + E_mean)
    a, b = sd_hat + eps, sd + eps
    inv_hat = 1.0 / a
    e_inv = E_sd / (a * b) + 2.0 * U64 / a
    e64 = e_d * inv_hat + d * e_inv + U64 * (d + e_d) * inv_hat
    out = d / b
    return (e64 + 2.0 * (2.0 ** -24 * (out + e64) + 2.0 ** -150)) * FP64_SLACK


def grad_norm_rel_bound(n):
    """-> the bound on |restatement - numpy.linalg.norm(A / count)| / norm over n parameters"""
    return (g(n + 4) + g(n + 2)) * FP64_SLACK


def clipped_norm_rel_bound(n):
    """-> the bound on |numpy.linalg.norm((A / count) * scale) - max_norm| / max_norm over n parameters, where the clip bites"""
    return (g(n + 4) + 2.0 * U64 + g(n + 2)) * FP64_SLACK


def adv_case(rows, n, seed, scale=1.0, masked=False):
    """advantages N(0.3 scale, scale**2) in f32 with a few exact zeros, and alive bytes (about one in five zero, or None)
    -> (adv float32 (rows, n), alive uint8 (rows, n) or None)"""
    rng = np.random.default_rng(9000 + seed)
    adv = (rng.normal(0.3, 1.0, (rows, n)) * scale).astype(np.float32)
    adv.reshape(-1)[rng.integers(0, rows * n, max(1, rows * n // 16))] = 0.0
    alive = (rng.uniform(size=(rows, n)) < 0.8).astype(np.uint8) if masked else None
    return adv, alive
