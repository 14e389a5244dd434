"""Error bounds of the policy's f32 arithmetic against an fp64 evaluation of the same f32 parameters, derived - not tuned - and
shared by tests/test_policy_host.py and tests/test_gpu_policy.py; and the seeded networks and inputs both use.  TEST CODE.

Notation: u = 2**-24 (unit roundoff of f32), gamma(n) = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms,
Lemma 3.1).  A dot product of K terms plus a bias, accumulated in ANY order with one rounding per operation (fused or not), has
|z_hat - z| <= gamma(K + 1) (|W| |h| + |b|) for exact inputs h (ibid. section 3.1); inputs that carry an error e_h of their own
add |W| e_h, and the rounding term is taken at |h| + e_h, the largest the computed inputs can be.
  input      x = fma(obs32, scale, shift): one rounding, e_x = u |x|
  relu       1-Lipschitz and exact: e_h = e_z
  tanh       1-Lipschitz, then the library function's own error: e_h = e_z + TAU_TANH ulp(h), ulp(h) <= 2 u |h|, at |h| + e_z
The library functions: the kernel calls tanhf / expf / logf of the ROCm device library (OCML), which implements the OpenCL C math
library; no accuracy table of its own ships with the toolchain, so the bounds are the OpenCL full-profile ones it has to meet
(OpenCL C 3.0 specification, section 7.4 "Relative error as ULPs": exp <= 3 ulp, log <= 3 ulp, tanh <= 5 ulp), with
1 ulp <= 2 u |result|.  IEEE division (hipcc's default: correctly rounded f32 divide) and addition: u each.
The fp64 reference's own rounding (2**-53 per operation, 2**-29 of u) is covered by the factor FP64_SLACK on every bound.
"""
import numpy as np

from basilisk_env_amd import policy as P

U = 2.0 ** -24
TAU_TANH, TAU_EXP, TAU_LOG = 5.0, 3.0, 3.0
FP64_SLACK = 1.0 + 2.0 ** -20


def gamma(n):
    return n * U / (1.0 - n * U)


def _net_bound(layers, activation, x, e_x):
    """fp64 forward pass of one network with the error bound carried along -> (z, e_z) of its output layer, each (out, n)."""
    h, e_h = x, e_x
    for li, (W, b) in enumerate(layers):
        W64, b64 = W.astype(np.float64), b.astype(np.float64)
        aW = np.abs(W64)
        z = W64 @ h + b64[:, None]
        e_z = gamma(W.shape[1] + 1) * (aW @ (np.abs(h) + e_h) + np.abs(b64)[:, None]) + aW @ e_h
        if li + 1 == len(layers):
            return z, e_z * FP64_SLACK
        if activation == "tanh":
            h = np.tanh(z)
            e_h = e_z + TAU_TANH * 2.0 * U * (np.abs(h) + e_z)
        else:
            h = np.maximum(z, 0.0)
            e_h = e_z


def mlp_bound(spec, params, obs):
    """-> logits64 (3, n), e_logits (3, n), value64 (n,) or None, e_value (n,) or None: the fp64 evaluation (``mlp_ref(fp64=True)``'s
    numbers) and the bound on |f32 chain - fp64| per output."""
    spec = P._as_spec(spec)
    scale, shift, a, v = P.unpack_params(spec, params)
    o32 = np.asarray(obs, np.float64).reshape(5, -1).astype(np.float32).astype(np.float64)
    x = o32 * scale.astype(np.float64)[:, None] + shift.astype(np.float64)[:, None]
    e_x = U * np.abs(x)
    l, e_l = _net_bound(a, spec.activation, x, e_x)
    if v is None:
        return l, e_l, None, None
    val, e_v = _net_bound(v, spec.value_activation, x, e_x)
    return l, e_l, val[0], e_v[0]


def softmax_bound(logits32):
    """For f32 logits that BOTH sides hold exactly: the fp64 CDF boundaries c0 = p_0, c1 = p_0 + p_1, the fp64 log-probabilities
    (3, n), and the bounds on the kernel's f32 versions: delta (n,) for both boundaries, e_logp (3, n).
      d_i = l_i - m           one subtraction: |d_hat - d| <= u |d|
      e_i = expf(d_hat)       exp(d_hat) = exp(d) exp(+-u |d|), then TAU_EXP ulp: relative error E_i
      s = (e_0 + e_1) + e_2   positive terms, two additions: relative error E_s <= (1 + max E)(1 + u)^2 - 1
      p_i = e_i / s           relative error E_p <= (1 + E_i)(1 + u) / (1 - E_s) - 1
      c1 = p_0 + p_1          one more addition
      logp_i = d_hat_i - logf(s_hat): log(s_hat) = log(s) + log(1 +- E_s), TAU_LOG ulp on it, one subtraction."""
    l = np.asarray(logits32, np.float32).reshape(3, -1).astype(np.float64)
    m = l.max(axis=0)
    d = l - m
    e = np.exp(d)
    s = e.sum(axis=0)
    p = e / s
    E = (1.0 + TAU_EXP * 2.0 * U) * np.exp(U * np.abs(d)) - 1.0
    E_s = (1.0 + E.max(axis=0)) * (1.0 + U) ** 2 - 1.0
    E_p = (1.0 + E) * (1.0 + U) / (1.0 - E_s) - 1.0
    d0 = p[0] * E_p[0]
    d1 = (d0 + p[1] * E_p[1]) * (1.0 + U) + U * (p[0] + p[1])
    delta = np.maximum(d0, d1) * FP64_SLACK
    logs = np.log(s)
    e_logs = -np.log1p(-E_s)
    e_logs = e_logs + TAU_LOG * 2.0 * U * (np.abs(logs) + e_logs)
    logp = d - logs
    e_logp = U * np.abs(d) + e_logs
    e_logp = (e_logp + U * (np.abs(logp) + e_logp)) * FP64_SLACK
    return p[0], p[0] + p[1], logp, delta, e_logp


IN_SCALE = np.array([2.0, 50.0, 1.5, 1.25, 0.75], np.float32)
IN_SHIFT = np.array([-0.5, 0.1, -0.3, -0.6, 0.2], np.float32)


def seeded_policy(hidden, activation="relu", value_hidden=None, seed=0, value_activation=None):
    """-> (Spec, params): weights N(0, 1 / fan_in), biases N(0, 0.1) (variances), the non-trivial input scale / shift above."""
    spec = P.check_spec(hidden, activation, value_hidden, value_activation)
    rng = np.random.default_rng(1000 + seed)

    def net(shapes):
        return [(rng.normal(0.0, np.sqrt(1.0 / i), (o, i)).astype(np.float32), rng.normal(0.0, np.sqrt(0.1), o).astype(np.float32))
                for o, i in shapes]
    a, v = P.layer_shapes(spec)
    return spec, P.pack_params(spec, net(a), None if v is None else net(v), IN_SCALE, IN_SHIFT)


def observation_like(n, seed=0):
    """(5, n) float64 in the ranges of the env's observation rows: |sigma_BR|, |omega| [rad/s], wheel-speed fraction, charge
    fraction, shadow factor."""
    rng = np.random.default_rng(2000 + seed)
    return np.stack([rng.uniform(0, 1.7, n), rng.uniform(0, 0.02, n), rng.uniform(0, 1.0, n), rng.uniform(0, 1.0, n),
                     np.where(rng.uniform(size=n) < 0.35, 0.0, 1.0) * np.where(rng.uniform(size=n) < 0.05, rng.uniform(size=n), 1.0)])


def centred(spec, params, obs):
    """The same policy with its output biases shifted so that the three logits have equal means over ``obs`` (5, n): a seeded
    network's biases otherwise let one action win almost everywhere, and a closed loop under a constant action tests little."""
    spec = P._as_spec(spec)
    scale, shift, a, v = P.unpack_params(spec, params)
    l, _ = P.mlp_ref(spec, params, obs, fp64=True)
    W, b = a[-1]
    a = a[:-1] + [(W, (b - l.mean(axis=1)).astype(np.float32))]
    return P.pack_params(spec, a, v, scale, shift)


def reset_observations(ic, cfg):
    """(5, n): the first observation of freshly reset envs, from their initial conditions (include/bskgpu.h: [|sigma_BN|, |omega|,
    |Omega| / limit, charge / 3600 / power_max, 1]) - near enough for ``centred``."""
    from basilisk_env_amd import _lib
    t = _lib.NF_BASE + cfg.n_rw
    return np.stack([np.linalg.norm(ic[6:9], axis=0), np.linalg.norm(ic[9:12], axis=0),
                     np.linalg.norm(ic[_lib.NF_BASE:t], axis=0) / cfg.wheel_limit, ic[t + _lib.T_CHARGE] / 3600.0 / cfg.power_max,
                     np.ones(ic.shape[1])])
