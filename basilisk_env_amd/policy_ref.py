"""The numpy restatements the policy, population and evolution-strategy kernels are held to, bit for bit: the oracle of this subsystem.

Each function repeats, operation by operation and in the kernel's order, what include/bskgpu.h defines: the networks (``mlp_ref``: every
layer output one k-ordered chain of ``fma32`` from the bias), the action choice (``act_ref``, ``softmax_ref``, the Philox draw of
``sample_uniform``), the per-member fitness of a rollout (``population_fitness_ref``), and the evolution strategy - its noise
(``es_noise_ref``: Philox, then Wichura's AS 241 with a series logarithm), members (``es_ask_ref``), ranking (``centred_ranks``) and the
SGD and Adam updates (``es_tell_ref``, ``es_tell_adam_ref``) and the same with a step size per parameter that adapts
(``es_ask_sigma_ref``, ``es_tell_pgpe_ref``) - with ``shared_slot_ref`` for the shared-episode reset, and the running
observation statistics with the input normalisation out of them (``obs_stats_accumulate_ref``, ``obs_stats_totals_ref``,
``obs_norm_ref``).
``EvolutionStrategy`` is the host-side search the device one was modelled on.  Needs numpy and ``policy_spec`` only: no device, no
library.  The tests compare these with the device for equality, so the order of operations and the ``np.errstate`` scopes are part
of what they state.
"""
import numpy as np

from .policy_spec import MODES, OUTCOME_COLS, OUTCOME_COLUMNS, _as_spec, check_sigma_adaptation, unpack_params

def fma32(a, b, c):
    """float32 arrays (broadcast against each other) -> float32: a * b + c rounded ONCE, what ``fmaf`` / ``v_fma_f32`` / one step
    of an f32 MFMA accumulator give.  The product of two float32 is exact in float64 (48 bits); TwoSum gives the exact residual of
    the float64 addition; the float64 sum is rounded to odd with it, and rounding that to float32 equals rounding the exact sum."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        t = s - p
        err = (p - (s - t)) + (c - t)                                        # TwoSum: s + err == p + c exactly
    s = np.ascontiguousarray(s)
    bits = s.view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s) & (s != 0)
    bits = np.where(fix, bits + np.where((err > 0) == (s > 0), 1, -1), bits)  # round to odd in 53 bits
    return np.where((s == 0) & (err != 0), err, bits.view(np.float64)).astype(np.float32)


def _forward32(layers, activation, x, chunk=2048):
    """the definition's chain, units x spacecraft; ``chunk`` spacecraft at a time (the working set stays in cache), the chunks
    spread over a few threads (numpy's array operations release the interpreter lock)"""
    n = x.shape[1]
    out = np.empty((layers[-1][0].shape[0], n), np.float32)

    def run(lo):
        h = x[:, lo:lo + chunk]
        for li, (W, b) in enumerate(layers):
            z = np.broadcast_to(b[:, None], (W.shape[0], h.shape[1])).astype(np.float32)
            for k in range(W.shape[1]):
                z = fma32(W[:, k:k + 1], h[k:k + 1, :], z)
            if li + 1 < len(layers):
                with np.errstate(invalid="ignore"):
                    z = np.tanh(z) if activation == "tanh" else np.where(z > 0, z, np.float32(0))
            h = z.astype(np.float32)
        out[:, lo:lo + chunk] = h
    starts = range(0, n, chunk)
    if len(starts) < 4:
        for lo in starts:
            run(lo)
    else:
        import os
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as pool:
            list(pool.map(run, starts))
    return out


def _forward64(layers, activation, x):
    h = x
    for li, (W, b) in enumerate(layers):
        h = W.astype(np.float64) @ h + b.astype(np.float64)[:, None]
        if li + 1 < len(layers):
            h = np.tanh(h) if activation == "tanh" else np.maximum(h, 0.0)
    return h


def mlp_ref(spec, params, obs, fp64=False):
    """numpy restatement of the policy's networks (include/bskgpu.h).  ``obs``: (5, n) float64 -> logits (3, n), value (n,) or None.
    Default: the definition itself - float32, every layer output one k-ordered ``fma32`` chain from the bias: bit for bit the
    kernel's logits and value for ``relu`` networks (``tanh`` is the host's here and the device library's there).
    ``fp64=True``: the same float32 parameters and float32-converted inputs carried through in float64 (what error bounds are
    derived against)."""
    spec = _as_spec(spec)
    scale, shift, a, v = unpack_params(spec, params)
    o32 = np.asarray(obs, np.float64).reshape(5, -1).astype(np.float32)
    if fp64:
        x = o32.astype(np.float64) * scale.astype(np.float64)[:, None] + shift.astype(np.float64)[:, None]
        return _forward64(a, spec.activation, x), (None if v is None else _forward64(v, spec.value_activation, x)[0])
    x = fma32(o32, scale[:, None], shift[:, None])
    return _forward32(a, spec.activation, x), (None if v is None else _forward32(v, spec.value_activation, x)[0])


_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_PHILOX_W0, _PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK32, _SH32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al. 2011) on uint64 arrays that hold 32-bit words -> the four output words (csrc/bsk_philox.hpp)."""
    c0, c1, c2, c3, k0, k1 = (np.asarray(w, np.uint64) for w in (c0, c1, c2, c3, k0, k1))
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> _SH32) ^ c1 ^ k0) & _MASK32, p1 & _MASK32, ((p0 >> _SH32) ^ c3 ^ k1) & _MASK32, p0 & _MASK32
        k0, k1 = (k0 + _PHILOX_W0) & _MASK32, (k1 + _PHILOX_W1) & _MASK32
    return c0, c1, c2, c3


def sample_uniform(n, seed=0, draw=0, env_base=0):
    """u of sample mode for spacecraft env_base .. env_base + n - 1: (w0 >> 8) * 2**-24 with w0 the first Philox word of counter
    (env_lo, env_hi, draw_lo, draw_hi) under key (seed_lo, seed_hi) -> float32 (n,)."""
    env = np.uint64(int(env_base)) + np.arange(int(n), dtype=np.uint64)
    seed, draw = np.uint64(int(seed)), np.uint64(int(draw))
    w0 = philox4x32_10(env & _MASK32, env >> _SH32, draw & _MASK32, draw >> _SH32, seed & _MASK32, seed >> _SH32)[0]
    return (w0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def softmax_ref(logits):
    """-> m, e (3, n), s of include/bskgpu.h step 5, float32 operations in the kernel's order (``exp`` is the host's)."""
    l = np.asarray(logits, np.float32).reshape(3, -1)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.fmax(np.fmax(l[0], l[1]), l[2])
        e = np.exp(l - m)
        s = (e[0] + e[1]) + e[2]
    return m, e, s


def act_ref(logits, mode="greedy", seed=0, draw=0, env_base=0):
    """numpy restatement of the action choice.  ``logits`` (3, n) float32 -> action int32 (n,), logp float32 (n,).
    greedy: the greatest logit, ties to the lowest index, a NaN loses to every number (three NaNs pick 0).
    sample: p_i = e_i / s, action = 0 if u < p_0, else 1 if u < p_0 + p_1, else 2 (``sample_uniform``)."""
    if mode not in MODES:
        raise ValueError("mode must be 'greedy' or 'sample'")
    l = np.asarray(logits, np.float32).reshape(3, -1)
    m, e, s = softmax_ref(l)
    if mode == "sample":
        u = sample_uniform(l.shape[1], seed, draw, env_base)
        with np.errstate(invalid="ignore", divide="ignore"):
            c0 = e[0] / s
            c1 = c0 + e[1] / s
        a = np.where(u < c0, 0, np.where(u < c1, 1, 2)).astype(np.int32)
    else:
        a = np.zeros(l.shape[1], np.int32)
        best = l[0].copy()
        for i in (1, 2):
            na, nb = np.isnan(l[i]), np.isnan(best)
            with np.errstate(invalid="ignore"):
                win = np.where(na != nb, nb, ~na & (l[i] > best))
            a[win] = i
            best[win] = l[i][win]
    with np.errstate(invalid="ignore", divide="ignore"):
        logp = (np.take_along_axis(l, a[None, :].astype(np.int64), axis=0)[0] - m) - np.log(s)
    return a, logp.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# Populations (bsk_population_*): the per-member fitness of a rollout, the ranking, and the host-side search around them

def population_fitness_ref(reward_hist, reason_hist, gamma, n_members):
    """numpy restatement of the device fitness (include/bskgpu.h).  ``reward_hist`` (T, n) float64, ``reason_hist`` (T, n): the
    rows a rollout records; n = n_members * E, E a multiple of 64.  -> dict: ``env_value`` (n,) float64 and ``env_len`` (n,) int32 -
    per env v = v + g * reward, len += 1, g = g * gamma while alive, alive until the first step with reason != 0 (included) - and
    ``fitness`` / ``mean_len`` (n_members,) float64: per member, lane l adds its elements l, l + 64, ... ascending from the first,
    then s[l] = s[l] + s[l + stride] for stride 32 ... 1, then s[0] / E.  Every operation rounds on its own, in the kernel's order:
    the results are equal bit for bit."""
    r = np.asarray(reward_hist, np.float64)
    q = np.asarray(reason_hist)
    if r.ndim != 2 or q.shape != r.shape:
        raise ValueError("reward_hist and reason_hist: (n_steps, n) each")
    n, P = r.shape[1], int(n_members)
    if P < 1 or n % P or (n // P) % 64 or n == 0:
        raise ValueError("n must be n_members * envs_per_member, envs_per_member a positive multiple of 64")
    E = n // P
    gamma = np.float64(gamma)
    v, g = np.zeros(n, np.float64), np.ones(n, np.float64)
    length, alive = np.zeros(n, np.int32), np.ones(n, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(r.shape[0]):
            p = g * r[t]
            v = np.where(alive, v + p, v)
            g = np.where(alive, g * gamma, g)
            length += alive
            alive &= q[t] == 0

        def mean(x):
            x = x.reshape(P, E // 64, 64)
            s = x[:, 0, :].copy()
            for i in range(1, E // 64):
                s = s + x[:, i, :]
            for stride in (32, 16, 8, 4, 2, 1):
                s[:, :stride] = s[:, :stride] + s[:, stride:2 * stride]
            return s[:, 0] / np.float64(E)
        return {"env_value": v, "env_len": length, "fitness": mean(v), "mean_len": mean(length.astype(np.float64))}


def _extreme_pick(m, x, greatest):
    """The rule of the outcome rows' minimum (``greatest``: maximum), elementwise: candidate x replaces incumbent m when it is
    smaller (greater) or the incumbent is a NaN.  The bits of whichever is kept are kept."""
    with np.errstate(invalid="ignore"):
        return np.where(((x > m) if greatest else (x < m)) | np.isnan(m), x, m)


def _extreme_lanes_then_tree(x, greatest):
    """That rule in the library's one order over the last axis of ``x`` (..., k): lane l = 0 .. 63 starts from the NaN that stands
    for "nothing yet" and takes its elements l, l + 64, ... ascending; then, for stride 32 ... 1, lane l + stride is the candidate
    against the incumbent in lane l.  -> (...,): lane 0."""
    x = np.asarray(x, np.float64)
    m = np.full(x.shape[:-1] + (64,), np.nan, np.float64)
    for at in range(0, x.shape[-1], 64):
        chunk = x[..., at:at + 64]
        m[..., :chunk.shape[-1]] = _extreme_pick(m[..., :chunk.shape[-1]], chunk, greatest)
    for stride in (32, 16, 8, 4, 2, 1):
        m[..., :stride] = _extreme_pick(m[..., :stride], m[..., stride:2 * stride], greatest)
    return m[..., 0]


def population_outcomes_ref(reward_hist, reason_hist, action_hist, gamma, E):
    """numpy restatement of the episode-outcome rows (include/bskgpu.h, bsk_population_set_outcomes) from the histories a rollout
    records: ``reward_hist`` (T, n) float64, ``reason_hist`` (T, n) and ``action_hist`` (T, n) integers, n = P * ``E``, E a multiple
    of 64.  -> float64 (P, 11), ``OUTCOME_COLUMNS``.  Per env, while alive before step t (``population_fitness_ref``'s rule):
    act_n[a_t] += 1 (an action outside 0..2 is counted nowhere), and end_reason = the reason byte of the step that ends the episode
    (0: never ended).  Per member: the envs whose end_reason has each of the four bits, the envs with end_reason 0, the three step
    counts - integers, converted once - then the sum of v * v (each product rounded on its own), the minimum and the maximum of v
    in the fitness's order: lanes ascending from the first element, then strides 32 ... 1.  Equal to the device bit for bit."""
    q = np.asarray(reason_hist)
    a = np.asarray(action_hist)
    E = int(E)
    if q.ndim != 2 or a.shape != q.shape:
        raise ValueError("reason_hist and action_hist: (n_steps, n) each")
    n = q.shape[1]
    if E < 64 or E % 64 or n == 0 or n % E:
        raise ValueError("n must be n_members * E, E a positive multiple of 64")
    P = n // E
    v = population_fitness_ref(reward_hist, q, gamma, P)["env_value"]
    act_n, end = np.zeros((3, n), np.int64), np.zeros(n, np.int64)
    alive = np.ones(n, bool)
    for t in range(q.shape[0]):
        for k in range(3):
            act_n[k] += alive & (a[t] == k)
        end = np.where(alive & (q[t] != 0), q[t].astype(np.int64), end)
        alive &= q[t] == 0
    rows = np.empty((P, OUTCOME_COLS), np.float64)
    for c, bit in enumerate((1, 2, 4, 8)):
        rows[:, c] = ((end & bit) != 0).reshape(P, E).sum(axis=1)
    rows[:, 4] = (end == 0).reshape(P, E).sum(axis=1)
    for k in range(3):
        rows[:, 5 + k] = act_n[k].reshape(P, E).sum(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (v * v).reshape(P, E // 64, 64)
        s = x[:, 0, :].copy()
        for i in range(1, E // 64):
            s = s + x[:, i, :]
        for stride in (32, 16, 8, 4, 2, 1):
            s[:, :stride] = s[:, :stride] + s[:, stride:2 * stride]
    rows[:, 8] = s[:, 0]
    rows[:, 9] = _extreme_lanes_then_tree(v.reshape(P, E), False)
    rows[:, 10] = _extreme_lanes_then_tree(v.reshape(P, E), True)
    return rows


def outcome_table_ref(rows):
    """Member rows float64 (..., 11) -> dict of arrays by ``OUTCOME_COLUMNS``: the eight counts as int64, the three value columns
    float64 as stored."""
    rows = np.asarray(rows, np.float64)
    if rows.shape[-1] != OUTCOME_COLS:
        raise ValueError("outcome rows have %d columns, got %r" % (OUTCOME_COLS, rows.shape))
    return {name: (rows[..., c].astype(np.int64) if c < 8 else rows[..., c].copy()) for c, name in enumerate(OUTCOME_COLUMNS)}


def centred_ranks(fitness):
    """(P,) fitness -> (P,) float64 utilities 0.5 (best) ... -0.5 (worst), evenly spaced.  The order is the library's ``beats`` rule
    (bsk_select_branches): the greater value first, a NaN below every number, equal values (and NaNs) to the lower index."""
    f = np.asarray(fitness, np.float64).reshape(-1)
    nan = np.isnan(f)
    order = np.lexsort((-np.where(nan, 0.0, f), nan))          # (stable: ties keep ascending index)
    u = np.empty(f.size, np.float64)
    u[order] = 0.5 - np.arange(f.size) / max(f.size - 1, 1)
    return u


class EvolutionStrategy(object):
    """A small antithetic evolution strategy with centred-rank utilities (Salimans et al. 2017, "Evolution Strategies as a Scalable
    Alternative to Reinforcement Learning"), host-side numpy: the piece that turns ``PolicyPopulation.evaluate`` into a search.
    ``ask()`` -> (P, n) float32 members theta + sigma * eps_i (even rows) and theta - sigma * eps_i (odd rows), P even;
    ``tell(fitness)`` moves theta by lr / (P * sigma) * sum_k u_k * (+-eps_k), u the ``centred_ranks`` of the fitness (greater is
    better).  The first ``frozen`` floats - a policy block's in_scale and in_shift - are never perturbed nor moved.  Seeded: the
    same seed asks the same members."""

    def __init__(self, theta, population, sigma=0.1, lr=0.05, seed=0, frozen=10):
        self.theta = np.array(theta, dtype=np.float64).reshape(-1)
        self.population, self.sigma, self.lr, self.frozen = int(population), float(sigma), float(lr), int(frozen)
        if self.population < 2 or self.population % 2:
            raise ValueError("population must be even and >= 2")
        if not (self.sigma > 0.0) or not (0 <= self.frozen <= self.theta.size):
            raise ValueError("sigma must be positive and frozen within the parameter block")
        self._rng = np.random.default_rng(seed)
        self._eps = None

    def ask(self):
        eps = self._rng.standard_normal((self.population // 2, self.theta.size))
        eps[:, :self.frozen] = 0.0
        self._eps = eps
        members = np.empty((self.population, self.theta.size), np.float64)
        members[0::2] = self.theta + self.sigma * eps
        members[1::2] = self.theta - self.sigma * eps
        return members.astype(np.float32)

    def tell(self, fitness):
        if self._eps is None:
            raise RuntimeError("tell() follows ask()")
        u = centred_ranks(fitness)
        if u.size != self.population:
            raise ValueError("expected %d fitness values, got %d" % (self.population, u.size))
        step = (u[0::2] - u[1::2]) @ self._eps
        self.theta = self.theta + self.lr / (self.population * self.sigma) * step
        self._eps = None
        return self.theta.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# The evolution strategy on the device (bsk_es_*; definition in include/bskgpu.h, kernels in csrc/bsk_es.hip), restated

# Wichura's AS 241 (PPND16), coefficients lowest first
_PPND_A = (3.3871328727963666080, 1.3314166789178437745e2, 1.9715909503065514427e3, 1.3731693765509461125e4,
           4.5921953931549871457e4, 6.7265770927008700853e4, 3.3430575583588128105e4, 2.5090809287301226727e3)
_PPND_B = (1.0, 4.2313330701600911252e1, 6.8718700749205790830e2, 5.3941960214247511077e3,
           2.1213794301586595867e4, 3.9307895800092710610e4, 2.8729085735721942674e4, 5.2264952788528545610e3)
_PPND_C = (1.42343711074968357734, 4.63033784615654529590, 5.76949722146069140550, 3.64784832476320460504,
           1.27045825245236838258, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
_PPND_D = (1.0, 2.05319162663775882187, 1.67638483018380384940, 6.89767334985100004550e-1,
           1.48103976427480074590e-1, 1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)
_PPND_E = (6.65790464350110377720, 5.46378491116411436990, 1.78482653991729133580, 2.96560571828504891230e-1,
           2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7)
_PPND_F = (1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2,
           7.86869131145613259100e-4, 1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15)


def _horner(coef, x):
    y = np.full_like(x, coef[-1])
    for c in coef[-2::-1]:
        y = y * x + c
    return y


def _series_log(p):
    """ln(p) of include/bskgpu.h for p in (0, 0.5): frexp, then the atanh series in (m - 1) / (m + 1) - no library logarithm"""
    m, e = np.frexp(p)
    low = m < 0.7071067811865476
    m = np.where(low, m + m, m)
    e = np.where(low, e - 1, e).astype(np.float64)
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    t = np.full_like(s, 1.0 / 23.0)
    for k in range(10, -1, -1):
        t = t * s2 + 1.0 / (2 * k + 1)
    return e * 0.6931471805599453 + (2.0 * s) * t


def es_uniform_ref(k):
    """52-bit integers k -> u = (k + 0.5) * 2**-52, exact and inside (0, 1)"""
    return (np.asarray(k, np.uint64).astype(np.float64) + 0.5) * 2.0 ** -52


def es_inverse_normal_ref(u):
    """The inverse normal CDF of include/bskgpu.h on float64 u in (0, 1): AS 241 with a series logarithm, every operation one of
    f64 + - * /, sqrt or an integer operation, each rounded on its own - the device's bits."""
    u = np.asarray(u, np.float64)
    q = u - 0.5
    centre = np.abs(q) <= 0.425
    r = 0.180625 - q * q
    z = q * _horner(_PPND_A, r) / _horner(_PPND_B, r)
    if not centre.all():
        tail = ~centre
        p = np.where(q[tail] < 0, u[tail], 1.0 - u[tail])
        r = np.sqrt(-_series_log(p))
        x, y = r - 1.6, r - 5.0
        t = np.where(r <= 5.0, _horner(_PPND_C, x) / _horner(_PPND_D, x), _horner(_PPND_E, y) / _horner(_PPND_F, y))
        z[tail] = np.where(q[tail] < 0, -t, t)
    return z


def es_noise_ref(seed, generation, pairs, n_params):
    """z(g, i, j) of include/bskgpu.h -> float64 (pairs, n_params): Philox4x32-10 under key (seed lo, seed hi) at counter
    (j, i, g lo, g hi); k = (w0 >> 6) * 2**26 + (w1 >> 6); u = (k + 0.5) * 2**-52; z = the inverse normal CDF of u."""
    seed, g = np.uint64(int(seed)), np.uint64(int(generation))
    j = np.broadcast_to(np.arange(int(n_params), dtype=np.uint64)[None, :], (int(pairs), int(n_params)))
    i = np.broadcast_to(np.arange(int(pairs), dtype=np.uint64)[:, None], j.shape)
    w0, w1, _, _ = philox4x32_10(j, i, g & _MASK32, g >> _SH32, seed & _MASK32, seed >> _SH32)
    k = ((w0 >> np.uint64(6)) << np.uint64(26)) + (w1 >> np.uint64(6))
    return es_inverse_normal_ref(es_uniform_ref(k))


def es_ask_ref(theta, sigma, frozen, P, seed, generation):
    """The members ``bsk_es_ask`` writes -> float32 (P, n_params): rows 2i / 2i + 1 are theta +- sigma * z(g, i, :), product and
    sum each rounded in float64, then rounded to float32; the first ``frozen`` columns are (float)theta."""
    theta = np.asarray(theta, np.float64).reshape(-1)
    P, frozen = int(P), int(frozen)
    step = np.float64(sigma) * es_noise_ref(seed, generation, P // 2, theta.size)
    step[:, :frozen] = 0.0
    members = np.empty((P, theta.size), np.float64)
    members[0::2] = theta + step
    members[1::2] = theta - step
    members[:, :frozen] = theta[:frozen]
    return members.astype(np.float32)


def es_tell_ref(theta, fitness, sigma, lr, frozen, seed, generation):
    """The theta ``bsk_es_tell`` leaves -> float64 (n_params,): w_i = u_2i - u_2i+1 of the ``centred_ranks``; per parameter
    j >= frozen lane l = 0 .. 63 sums w_i * z(g, i, j) over its pairs i = l, l + 64, ... ascending from the first (+0.0 with no
    pair), the lanes join as the fitness tree does (stride 32 ... 1), and theta_j = theta_j + lr / (P * sigma) * s[0]."""
    theta = np.array(theta, dtype=np.float64).reshape(-1)
    frozen = int(frozen)
    s0, P = _es_pair_sum(fitness, theta.size, seed, generation)
    with np.errstate(invalid="ignore", over="ignore"):
        c = float(lr) / (float(P) * float(sigma))
        theta[frozen:] = theta[frozen:] + c * s0[frozen:]
    return theta


def _es_pair_sums(fitness, n_params, seed, generation, with_r=False):
    """Steps 1 - 3 of ``bsk_es_tell`` up to the sums -> (s0, r0, P), float64 (n_params,) each: the ONE helper behind every tell
    restatement.  s0 is over w_i * z, w_i = u_2i - u_2i+1; r0 (``with_r``; None otherwise) is over q_i * (z * z - 1.0),
    q_i = u_2i + u_2i+1, from the same z.  Each sum in the one order: lane l = 0 .. 63 takes its pairs l, l + 64, ... ascending from
    the first (+0.0 with none), then the lanes join in the tree with strides 32 ... 1."""
    u = centred_ranks(fitness)
    P = u.size
    if P < 2 or P % 2:
        raise ValueError("expected an even number of fitness values, at least 2")
    z = es_noise_ref(seed, generation, P // 2, n_params)

    def lanes_then_tree(terms):
        s = np.zeros((64, int(n_params)), np.float64)
        s[:min(64, P // 2)] = terms[:64]
        for at in range(64, P // 2, 64):
            chunk = terms[at:at + 64]
            s[:len(chunk)] = s[:len(chunk)] + chunk
        for stride in (32, 16, 8, 4, 2, 1):
            s[:stride] = s[:stride] + s[stride:2 * stride]
        return s[0].copy()
    with np.errstate(invalid="ignore", over="ignore"):
        s0 = lanes_then_tree((u[0::2] - u[1::2])[:, None] * z)
        r0 = lanes_then_tree((u[0::2] + u[1::2])[:, None] * (z * z - 1.0)) if with_r else None
    return s0, r0, P


def _es_pair_sum(fitness, n_params, seed, generation):
    """-> (s0, P) of ``_es_pair_sums``: the sum behind ``es_tell_ref`` and ``es_tell_adam_ref``, as ``ES_PAIR_SUM`` (csrc/bsk_es.hip)
    is behind the two update kernels."""
    s0, _, P = _es_pair_sums(fitness, n_params, seed, generation)
    return s0, P


def check_adam(beta1, beta2, eps, weight_decay):
    """The argument rules of ``bsk_es_set_optimizer(BSK_ES_ADAM, ...)`` -> the four as floats; ValueError where it returns
    BSK_EINVAL.  Needs no device."""
    beta1, beta2, eps, weight_decay = float(beta1), float(beta2), float(eps), float(weight_decay)
    if not (0.0 <= beta1 < 1.0) or not (0.0 <= beta2 < 1.0):
        raise ValueError("beta1 and beta2 must be in [0, 1)")
    if not np.isfinite(eps) or not (eps > 0.0):
        raise ValueError("eps must be finite and positive")
    if not np.isfinite(weight_decay) or weight_decay < 0.0:
        raise ValueError("weight_decay must be finite and not negative")
    return beta1, beta2, eps, weight_decay


def _adam_step_ref(m, v, beta_pow, g, lr, b1, b2, eps):
    """Adam's lines of include/bskgpu.h (csrc/bsk_es.hpp: adam_step) on float64 arrays, every operation rounded on its own
    -> (m, v, step, beta_pow moved on): m = b1 m + (1 - b1) g; v = b2 v + ((1 - b2) g) g;
    step = (lr * (m / (1 - p1))) / (sqrt(v / (1 - p2)) + eps) with p = beta_pow * beta.  The evolution strategy adds the step to
    theta, the policy fit subtracts it.  The caller holds the ``np.errstate`` scope."""
    one = np.float64(1.0)
    a1, a2 = one - b1, one - b2
    p1, p2 = beta_pow[0] * b1, beta_pow[1] * b2
    mj = b1 * m + a1 * g
    vj = b2 * v + (a2 * g) * g
    return mj, vj, (lr * (mj / (one - p1))) / (np.sqrt(vj / (one - p2)) + eps), np.array([p1, p2], np.float64)


def es_tell_adam_ref(theta, m, v, beta_pow, fitness, sigma, lr, frozen, seed, generation, beta1, beta2, eps, weight_decay):
    """What ``bsk_es_tell`` leaves under ``BSK_ES_ADAM`` -> (theta, m, v, beta_pow), float64: s[0] of ``es_tell_ref``'s sum, then
    per parameter j >= frozen, every operation rounded on its own (include/bskgpu.h), cg = 1 / (P * sigma):
    g = cg * s[0] - weight_decay * theta_j; m_j = beta1 * m_j + (1 - beta1) * g; v_j = beta2 * v_j + ((1 - beta2) * g) * g;
    theta_j = theta_j + (lr * (m_j / (1 - p1))) / (sqrt(v_j / (1 - p2)) + eps) with p = beta_pow * beta, the beta_pow returned."""
    theta = np.array(theta, dtype=np.float64).reshape(-1)
    m, v = np.array(m, dtype=np.float64).reshape(-1), np.array(v, dtype=np.float64).reshape(-1)
    bp = np.array(beta_pow, dtype=np.float64).reshape(2)
    frozen = int(frozen)
    if m.size != theta.size or v.size != theta.size:
        raise ValueError("m and v have theta's size")
    b1, b2, eps, wd = (np.float64(x) for x in check_adam(beta1, beta2, eps, weight_decay))
    s0, P = _es_pair_sum(fitness, theta.size, seed, generation)
    lr = np.float64(lr)
    cg = np.float64(1.0) / (np.float64(P) * np.float64(sigma))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = theta[frozen:]
        m[frozen:], v[frozen:], step, bp = _adam_step_ref(m[frozen:], v[frozen:], bp, cg * s0[frozen:] - wd * t, lr, b1, b2, eps)
        theta[frozen:] = t + step
    return theta, m, v, bp


def es_ask_sigma_ref(theta, sigma_vec, frozen, P, seed, generation):
    """The members ``bsk_es_ask`` writes under ``BSK_ES_SIGMA_PGPE`` -> float32 (P, n_params): ``es_ask_ref`` with sigma_vec[j] in
    the place of sigma.  The first ``frozen`` entries of ``sigma_vec`` are not read."""
    theta = np.asarray(theta, np.float64).reshape(-1)
    sv = np.asarray(sigma_vec, np.float64).reshape(-1)
    if sv.size != theta.size:
        raise ValueError("sigma_vec has theta's size")
    P, frozen = int(P), int(frozen)
    step = sv[None, :] * es_noise_ref(seed, generation, P // 2, theta.size)
    step[:, :frozen] = 0.0
    members = np.empty((P, theta.size), np.float64)
    members[0::2] = theta + step
    members[1::2] = theta - step
    members[:, :frozen] = theta[:frozen]
    return members.astype(np.float32)


def es_tell_pgpe_ref(theta, sigma_vec, fitness, lr, frozen, seed, generation, lr_sigma, max_change, sigma_min, sigma_max, adam=None):
    """What ``bsk_es_tell`` leaves under ``BSK_ES_SIGMA_PGPE`` (include/bskgpu.h), float64 -> (theta, sigma_vec), or with
    ``adam=(m, v, beta_pow, beta1, beta2, eps, weight_decay)`` -> (theta, sigma_vec, m, v, beta_pow).  Both sums from
    ``_es_pair_sums``; per parameter j >= frozen with sg = sigma_vec[j] as given and Pd = float(P), every operation rounded on its
    own: SGD theta_j = theta_j + (lr / (Pd * sg)) * s[0]; Adam ``es_tell_adam_ref``'s rule with cg = 1 / (Pd * sg);
    d = (cs * r[0]) * sg with cs = lr_sigma / Pd, clamped to +- max_change * sg; sigma_vec[j] = sg + d clamped to
    [sigma_min, sigma_max].  ``sigma_vec`` need not lie inside the bounds (``bsk_es_set_sigma`` takes any positive vector)."""
    theta = np.array(theta, dtype=np.float64).reshape(-1)
    sv = np.array(sigma_vec, dtype=np.float64).reshape(-1)
    frozen = int(frozen)
    if sv.size != theta.size:
        raise ValueError("sigma_vec has theta's size")
    if not (np.isfinite(sv).all() and (sv > 0.0).all()):
        raise ValueError("every entry of sigma_vec must be finite and positive")
    lr_sigma, max_change, sigma_min, sigma_max = (np.float64(x) for x in check_sigma_adaptation(lr_sigma, max_change, sigma_min, sigma_max))
    s0, r0, P = _es_pair_sums(fitness, theta.size, seed, generation, with_r=True)
    pd, lr = np.float64(P), np.float64(lr)
    cs = lr_sigma / pd
    sg, t = sv[frozen:], theta[frozen:]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if adam is None:
            theta[frozen:] = t + (lr / (pd * sg)) * s0[frozen:]
        else:
            m, v, beta_pow, beta1, beta2, eps, weight_decay = adam
            m, v = np.array(m, dtype=np.float64).reshape(-1), np.array(v, dtype=np.float64).reshape(-1)
            bp = np.array(beta_pow, dtype=np.float64).reshape(2)
            if m.size != theta.size or v.size != theta.size:
                raise ValueError("m and v have theta's size")
            b1, b2, eps, wd = (np.float64(x) for x in check_adam(beta1, beta2, eps, weight_decay))
            cg = np.float64(1.0) / (pd * sg)
            m[frozen:], v[frozen:], step, bp = _adam_step_ref(m[frozen:], v[frozen:], bp, cg * s0[frozen:] - wd * t, lr, b1, b2, eps)
            theta[frozen:] = t + step
        d = (cs * r0[frozen:]) * sg
        lim = max_change * sg
        d = np.where(d > lim, lim, np.where(d < -lim, -lim, d))
        n = sg + d
        n = np.where(n < sigma_min, sigma_min, n)
        n = np.where(n > sigma_max, sigma_max, n)
        sv[frozen:] = n
    if adam is None:
        return theta, sv
    return theta, sv, m, v, bp


# The training log and the champion (bsk_es_set_log; kernels es_log_kernel / es_best_kernel), restated

ES_LOG_COLUMNS = ("best", "worst", "sum", "sum_sq", "count", "best_member", "len_sum", "best_len")
ES_LOG_EMPTY = 2 ** 64 - 1                     # log_gen of a slot that has never been written, best_generation of no champion


def _lanes_then_tree(x):
    """The library's one order on a 1-D float64 array -> s[0]: lane l = 0 .. 63 adds its elements l, l + 64, ... ascending from the
    first (+0.0 with none), then s[l] = s[l] + s[l + stride] for stride 32 ... 1."""
    x = np.asarray(x, np.float64).reshape(-1)
    s = np.zeros(64, np.float64)
    s[:min(64, x.size)] = x[:64]
    with np.errstate(invalid="ignore", over="ignore"):
        for at in range(64, x.size, 64):
            chunk = x[at:at + 64]
            s[:chunk.size] = s[:chunk.size] + chunk
        for stride in _TREE:
            s[:stride] = s[:stride] + s[stride:2 * stride]
    return s[0]


def es_log_order_ref(fitness):
    """-> (b, wst) of include/bskgpu.h under the order of ``centred_ranks``: b the member nobody beats; wst, among the members
    that are not NaN, the one that beats no other of them (-1 when all are NaN)."""
    f = np.asarray(fitness, np.float64).reshape(-1)
    nan = np.isnan(f)
    order = np.lexsort((-np.where(nan, 0.0, f), nan))          # (centred_ranks' order: the best first, NaNs last)
    cnt = int(f.size - nan.sum())
    return int(order[0]), (int(order[cnt - 1]) if cnt else -1)


def es_log_row_ref(fitness, mean_len=None):
    """The eight words ``bsk_es_tell`` writes into its log row -> float64 (8,), ``ES_LOG_COLUMNS``: f[b], f[wst] (NaN when every
    member is NaN), S1 over x_k = f_k (+0.0 for a NaN), S2 over x_k * x_k, the number of non-NaN members, b, and with ``mean_len``
    (P,) L1 over it and mean_len[b] (+0.0 both without) - each sum in the library's one order, every operation rounded on its own."""
    f = np.asarray(fitness, np.float64).reshape(-1)
    if f.size < 1:
        raise ValueError("expected at least one fitness value")
    b, wst = es_log_order_ref(f)
    nan = np.isnan(f)
    x = np.where(nan, 0.0, f)
    with np.errstate(invalid="ignore", over="ignore"):
        q = x * x
    row = np.zeros(8, np.float64)
    row[0] = f[b]
    row[1] = f[wst] if wst >= 0 else np.nan
    row[2], row[3] = _lanes_then_tree(x), _lanes_then_tree(q)
    row[4], row[5] = float(f.size - nan.sum()), float(b)
    if mean_len is not None:
        ml = np.asarray(mean_len, np.float64).reshape(-1)
        if ml.size != f.size:
            raise ValueError("mean_len has one value per member")
        row[6], row[7] = _lanes_then_tree(ml), ml[b]
    return row


def es_log_slot_ref(generation, capacity):
    """The ring slot of a generation: the whole 64-bit word mod the capacity."""
    if int(capacity) < 1:
        raise ValueError("capacity must be >= 1")
    return (int(generation) & (2 ** 64 - 1)) % int(capacity)


def es_champion_empty(n_params):
    """The champion after ``bsk_es_set_log`` -> (params float32 zeros, fitness NaN, generation all ones, member -1)."""
    return np.zeros(int(n_params), np.float32), float("nan"), ES_LOG_EMPTY, -1


def es_best_ref(champion, fitness, generation, members_row_fn):
    """The champion rule of ``bsk_es_tell`` -> the new (params, fitness, generation, member).  ``champion``: the old four;
    ``members_row_fn(b)`` -> member b of this generation as ask writes it, float32 (n_params,) - a row of ``es_ask_ref`` /
    ``es_ask_sigma_ref`` on theta and sigma as they are BEFORE this tell (there is no second noise formula here); called only when
    the generation's best member takes: it is not NaN and the champion is NaN or strictly lower.  A tie keeps the older one."""
    params, best, gen, member = champion
    f = np.asarray(fitness, np.float64).reshape(-1)
    b, _ = es_log_order_ref(f)
    fb = float(f[b])
    if np.isnan(fb) or not (np.isnan(best) or fb > best):
        return np.array(params, np.float32), float(best), int(gen), int(member)
    return np.array(members_row_fn(b), dtype=np.float32).reshape(-1), fb, int(generation) & (2 ** 64 - 1), b


def es_log_table_ref(gen, rows):
    """The ring as ``bsk_es_get_log`` returns it -> ``training_log``'s dict of numpy arrays over the slots that have been written,
    sorted by generation: ``generation`` uint64, ``ES_LOG_COLUMNS`` (float64; ``count`` and ``best_member`` int64), and derived on
    the host ``mean`` = sum / count and ``std`` = sqrt(max(sum_sq / count - mean * mean, 0)), NaN where count == 0."""
    gen = np.asarray(gen, np.uint64).reshape(-1)
    rows = np.asarray(rows, np.float64).reshape(gen.size, 8)
    valid = np.flatnonzero(gen != np.uint64(ES_LOG_EMPTY))
    valid = valid[np.argsort(gen[valid], kind="stable")]
    out = {"generation": gen[valid].copy()}
    for c, name in enumerate(ES_LOG_COLUMNS):
        col = rows[valid, c].copy()
        out[name] = col.astype(np.int64) if name in ("count", "best_member") else col
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        n = np.where(out["count"] > 0, out["count"], 1).astype(np.float64)
        mean = out["sum"] / n
        var = out["sum_sq"] / n - mean * mean
        std = np.sqrt(np.where(var > 0, var, 0.0))
    out["mean"] = np.where(out["count"] > 0, mean, np.nan)
    out["std"] = np.where(out["count"] > 0, std, np.nan)
    return out


# The outcome ring (bsk_es_set_outcome_log; kernel es_outcome_kernel), restated

def _outcome_totals(rows):
    """Block A / C of an outcome row over member rows (k, 11) -> float64 (11,): the counts summed as integers, column 8 in the
    library's one order, columns 9 and 10 under the rows' own rule in that order; +0.0 everywhere with no member."""
    out = np.zeros(OUTCOME_COLS, np.float64)
    if rows.shape[0] == 0:
        return out
    with np.errstate(invalid="ignore"):
        out[:8] = rows[:, :8].astype(np.int64).sum(axis=0)
    out[8] = _lanes_then_tree(rows[:, 8])
    out[9] = _extreme_lanes_then_tree(rows[:, 9], False)
    out[10] = _extreme_lanes_then_tree(rows[:, 10], True)
    return out


def es_outcome_row_ref(member_rows, fitness, P, V):
    """The 33 words ``bsk_es_tell`` writes into its outcome ring -> float64 (33,): the totals over the P ranked members' rows, the
    row of the member the ranking puts first (``es_log_order_ref``'s b), the totals over the V validation members' rows (+0.0 with
    V = 0).  ``member_rows``: (P + V, 11) as the rollout wrote them; ``fitness``: at least P values, of which the first P rank."""
    P, V = int(P), int(V)
    rows = np.asarray(member_rows, np.float64)
    f = np.asarray(fitness, np.float64).reshape(-1)
    if P < 1 or V < 0 or rows.shape != (P + V, OUTCOME_COLS) or f.size < P:
        raise ValueError("member_rows: (P + V, %d) and at least P fitness values" % OUTCOME_COLS)
    b, _ = es_log_order_ref(f[:P])
    return np.concatenate([_outcome_totals(rows[:P]), rows[b], _outcome_totals(rows[P:])])


def es_outcome_table_ref(gen, rows):
    """The ring as ``bsk_es_get_outcome_log`` returns it -> ``outcome_log``'s dict over the slots that have been written, sorted by
    generation: ``generation`` uint64, and ``members`` / ``best`` / ``validation``, each an ``outcome_table_ref`` dict of arrays
    over those generations."""
    gen = np.asarray(gen, np.uint64).reshape(-1)
    rows = np.asarray(rows, np.float64).reshape(gen.size, 3, OUTCOME_COLS)
    valid = np.flatnonzero(gen != np.uint64(ES_LOG_EMPTY))
    valid = valid[np.argsort(gen[valid], kind="stable")]
    out = {"generation": gen[valid].copy()}
    for k, name in enumerate(("members", "best", "validation")):
        out[name] = outcome_table_ref(rows[valid, k])
    return out


def check_log(capacity, population=None, mean_len_size=None):
    """The argument rules of ``set_log`` that need no device -> the capacity as an int; ValueError where ``bsk_es_set_log`` returns
    BSK_EINVAL or the bound array does not have one float64 per member."""
    if isinstance(capacity, bool) or int(capacity) != capacity:
        raise ValueError("log capacity must be an integer, got %r" % (capacity,))
    capacity = int(capacity)
    if capacity < 0 or capacity > 2 ** 31 - 1:
        raise ValueError("log capacity must be in 0..2^31-1, got %d" % capacity)
    if mean_len_size is not None and population is not None and int(mean_len_size) != int(population):
        raise ValueError("mean_len: %d contiguous float64, got %d" % (int(population), int(mean_len_size)))
    return capacity


# Validation on fixed episodes (bsk_es_set_validation; kernels es_center_kernel / es_validate_kernel / es_val_best_kernel), restated

ES_VAL_COLUMNS = ("fitness", "mean_len", "take", "members")
ES_VAL_MAX_MEMBERS = 16


def check_validation(members, capacity=None, epoch=0, log_capacity=0):
    """The argument rules of ``set_validation`` that need no device -> (members, capacity, epoch) as ints; ValueError where
    ``bsk_es_set_validation`` returns BSK_EINVAL.  ``capacity`` None: the log's capacity, or 64 with no log."""
    for what, x in (("validation members", members), ("validation epoch", epoch)) + ((("validation capacity", capacity),) if capacity is not None else ()):
        if isinstance(x, bool) or int(x) != x:
            raise ValueError("%s must be an integer, got %r" % (what, x))
    members, epoch = int(members), int(epoch)
    if members < 0 or members > ES_VAL_MAX_MEMBERS:
        raise ValueError("validation members must be in 0..%d, got %d" % (ES_VAL_MAX_MEMBERS, members))
    capacity = (int(log_capacity) or 64) if capacity is None else int(capacity)
    if members and (capacity < 1 or capacity > 2 ** 31 - 1):
        raise ValueError("validation capacity must be in 1..2^31-1, got %d" % capacity)
    if epoch < 0 or epoch > 2 ** 64 - 1 - ES_VAL_MAX_MEMBERS:
        raise ValueError("validation epoch must be in 0..2^64-17, got %d" % epoch)
    return members, capacity, epoch


def es_center_ref(theta):
    """What ``bsk_es_ask`` writes into every validation member -> float32 (n_params,), the C-ABI parameter block: the plain
    (float)theta_j of every j, frozen or not - no ``+ sigma * 0``, so a -0.0 in theta stays -0.0."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(theta, np.float64).reshape(-1).astype(np.float32)


def es_validation_state(members, capacity, n_params, epoch=0):
    """The validation state after ``bsk_es_set_validation`` -> dict: ``epochs`` uint64 (V,) = epoch + v, ``gen`` uint64 (C,) all
    ones, ``rows`` float64 (C, 4) zeros, ``best_params`` float32 zeros, ``best_fitness`` NaN, ``best_generation`` all ones,
    ``take`` 0."""
    V, C = int(members), int(capacity)
    if V < 1 or V > ES_VAL_MAX_MEMBERS or C < 1:
        raise ValueError("members in 1..%d and capacity >= 1" % ES_VAL_MAX_MEMBERS)
    return {"epochs": np.array([(int(epoch) + v) & (2 ** 64 - 1) for v in range(V)], np.uint64),
            "gen": np.full(C, ES_LOG_EMPTY, np.uint64), "rows": np.zeros((C, 4), np.float64),
            "best_params": np.zeros(int(n_params), np.float32), "best_fitness": float("nan"), "best_generation": ES_LOG_EMPTY, "take": 0}


def es_validate_ref(state, fitness, mean_len, generation, theta):
    """The two validation launches of ``bsk_es_tell`` -> the new state (``es_validation_state``'s dict; the old one is not touched).
    ``fitness``: float64 (P + V,) - its LAST V = len(state["epochs"]) values are the validation members'; ``mean_len``: the same
    shape or None (nothing bound: L_c = +0.0); ``theta``: float64 (n_params,) as ask read it.  s = f[P], then + f[P + v] for v
    ascending, f_c = s / V, L_c likewise; the champion rule on f_c - not NaN, and the champion NaN or strictly lower: a tie keeps
    the older one; row g mod C = {f_c, L_c, take, V}; with take the champion's floats are ``es_center_ref(theta)``."""
    V, C = len(state["epochs"]), len(state["gen"])
    f = np.asarray(fitness, np.float64).reshape(-1)
    if f.size < V:
        raise ValueError("expected at least %d fitness values" % V)
    g = int(generation) & (2 ** 64 - 1)

    def centre(x):
        x = np.asarray(x, np.float64).reshape(-1)
        if x.size != f.size:
            raise ValueError("mean_len has one value per member")
        with np.errstate(invalid="ignore", over="ignore"):
            s = np.float64(x[x.size - V])
            for v in range(1, V):
                s = np.float64(s + x[x.size - V + v])
            return np.float64(s / np.float64(V))
    fc = centre(f)
    lc = np.float64(0.0) if mean_len is None else centre(mean_len)
    best = state["best_fitness"]
    take = (not np.isnan(fc)) and (np.isnan(best) or fc > best)
    out = {"epochs": state["epochs"].copy(), "gen": state["gen"].copy(), "rows": state["rows"].copy(),
           "best_params": state["best_params"].copy(), "best_fitness": best, "best_generation": state["best_generation"],
           "take": 1 if take else 0}
    slot = g % C
    out["rows"][slot] = (fc, lc, 1.0 if take else 0.0, float(V))
    out["gen"][slot] = np.uint64(g)
    if take:
        out["best_fitness"], out["best_generation"], out["best_params"] = float(fc), g, es_center_ref(theta)
    return out


def es_validation_table_ref(gen, rows):
    """The ring as ``bsk_es_get_validation_log`` returns it -> ``validation_log``'s dict of numpy arrays over the slots that have
    been written, sorted by generation: ``generation`` uint64 and ``ES_VAL_COLUMNS`` (float64; ``take`` and ``members`` int64)."""
    gen = np.asarray(gen, np.uint64).reshape(-1)
    rows = np.asarray(rows, np.float64).reshape(gen.size, 4)
    valid = np.flatnonzero(gen != np.uint64(ES_LOG_EMPTY))
    valid = valid[np.argsort(gen[valid], kind="stable")]
    out = {"generation": gen[valid].copy()}
    for c, name in enumerate(ES_VAL_COLUMNS):
        col = rows[valid, c].copy()
        out[name] = col.astype(np.int64) if name in ("take", "members") else col
    return out


def shared_slot_ref(n, envs_per_member, epoch, n_pool, env_base=0):
    """The IC-pool slots ``bsk_reset_from_pool_shared`` restarts envs 0 .. n - 1 from -> uint32 (n,): g = (env_base + env) mod 2^32,
    q = g mod envs_per_member, e = epoch mod 2^32, slot = (q * 2654435761 + e * 40503 + 12345) mod 2^32 mod n_pool.  Envs with equal
    q share a slot.  Needs no device."""
    n, E, n_pool = int(n), int(envs_per_member), int(n_pool)
    if E < 1 or n_pool < 1:
        raise ValueError("envs_per_member and n_pool must be >= 1")
    mask = np.uint64(0xFFFFFFFF)
    g = (np.arange(n, dtype=np.uint64) + np.uint64(int(env_base) & 0xFFFFFFFF)) & mask
    q = g % np.uint64(E)
    e = np.uint64(int(epoch) & 0xFFFFFFFF)
    return (((q * np.uint64(2654435761) + e * np.uint64(40503) + np.uint64(12345)) & mask) % np.uint64(n_pool)).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# Running observation statistics (bsk_obs_stats_*; definition in include/bskgpu.h, kernels in csrc/bsk_obsstats.hip), restated

_TREE = (32, 16, 8, 4, 2, 1)


def obs_stats_zero_state(n_cap):
    """The state of a new statistics object of capacity ``n_cap`` -> (part float64 (W, 10), cnt uint64 (W,)), W = ceil(n_cap / 64)."""
    W = (int(n_cap) + 63) // 64
    if W < 1:
        raise ValueError("n_cap must be >= 1")
    return np.zeros((W, 10), np.float64), np.zeros(W, np.uint64)


def obs_stats_accumulate_ref(state, obs5n, alive=None):
    """One ``bsk_obs_stats_accumulate`` -> the new (part, cnt); ``state`` is not changed.  ``obs5n`` (5, n) float64, ``alive`` (n,) or
    None (every spacecraft counts).  Wave w is the spacecraft 64 w .. 64 w + 63; a lane that does not count brings +0.0; x and
    x * x each go through the fitness tree (stride 32 ... 1) and the wave's ten sums are added to part[w], the number of counting
    lanes to cnt[w]; a wave in which no lane counts is left alone."""
    part, cnt = np.array(state[0], dtype=np.float64), np.array(state[1], dtype=np.uint64)
    obs = np.asarray(obs5n, np.float64)
    if part.ndim != 2 or part.shape[1] != 10 or cnt.shape != (part.shape[0],):
        raise ValueError("state: part (W, 10) and cnt (W,)")
    if obs.ndim != 2 or obs.shape[0] != 5 or not (1 <= obs.shape[1] <= 64 * part.shape[0]):
        raise ValueError("observations: (5, n) with 1 <= n <= 64 * W")
    n = obs.shape[1]
    counts = np.ones(n, bool) if alive is None else np.asarray(alive).reshape(-1) != 0
    if counts.size != n:
        raise ValueError("alive: one byte per spacecraft")
    nw = (n + 63) // 64
    x = np.zeros((5, nw * 64), np.float64)
    x[:, :n] = np.where(counts, obs, 0.0)
    lanes = np.zeros(nw * 64, bool)
    lanes[:n] = counts
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = np.concatenate([x, x * x]).reshape(10, nw, 64)
        for stride in _TREE:
            s[:, :, :stride] = s[:, :, :stride] + s[:, :, stride:2 * stride]
        live = lanes.reshape(nw, 64).sum(axis=1)
        stores = np.flatnonzero(live > 0)
        part[stores] = part[stores] + s[:, stores, 0].T
    cnt[:nw] = cnt[:nw] + live.astype(np.uint64)
    return part, cnt


def obs_stats_totals_ref(state):
    """The join -> (tot float64 (10,), count int): per column lane l adds part[w] for w = l, l + 64, ... ascending from the first
    (+0.0 with no element), the lanes join in the fitness tree; count is the sum of cnt."""
    part, cnt = np.asarray(state[0], np.float64), np.asarray(state[1], np.uint64)
    W = part.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros((64, 10), np.float64)
        s[:min(64, W)] = part[:64]
        for at in range(64, W, 64):
            chunk = part[at:at + 64]
            s[:len(chunk)] = s[:len(chunk)] + chunk
        for stride in _TREE:
            s[:stride] = s[:stride] + s[stride:2 * stride]
    return s[0].copy(), sum(int(c) for c in cnt)


def obs_moments_ref(tot, count):
    """-> (mean, var) float64 (5,) each of count > 0 observations: mean = tot[k] / N, var = max(tot[5 + k] / N - mean * mean, 0)."""
    tot = np.asarray(tot, np.float64).reshape(10)
    N = np.float64(int(count))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        mean = tot[:5] / N
        var = tot[5:] / N - mean * mean
    return mean, np.where(var > 0, var, 0.0)


def obs_norm_ref(tot, count, std_min):
    """What ``bsk_es_apply_obs_norm`` writes -> (in_scale, in_shift) float64 (5,) each, or None while count == 0 (nothing is
    written): sd = sqrt(var), scale = 1 / sd where sd >= std_min and 0 elsewhere - a row that has not varied is switched off, the
    rule of ARS - and shift = 0 - mean * scale."""
    if int(count) == 0:
        return None
    mean, var = obs_moments_ref(tot, count)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        sd = np.sqrt(var)
        scale = np.where(sd >= np.float64(std_min), np.float64(1.0) / sd, 0.0)
        shift = np.float64(0.0) - mean * scale
    return scale, shift


# ---------------------------------------------------------------------------------------------------------------------------------
# Fitting the policy to labelled observations (bsk_fit_*; definition in include/bskgpu.h, kernels in csrc/bsk_fit.hip), restated

FIT_BLOCK = 64                                 # samples of one gradient block
FIT_STATS_COLUMNS = ("nll_sum", "value_loss_sum", "correct", "count")


def check_fit(lr, beta1, beta2, eps, weight_decay, value_coef):
    """The argument rules of ``bsk_fit_create`` -> the six as floats; ValueError where it returns BSK_EINVAL.  Needs no device."""
    lr, value_coef = float(lr), float(value_coef)
    if not np.isfinite(lr) or lr < 0.0:
        raise ValueError("lr must be finite and not negative")
    beta1, beta2, eps, weight_decay = check_adam(beta1, beta2, eps, weight_decay)
    if not np.isfinite(value_coef) or value_coef < 0.0:
        raise ValueError("value_coef must be finite and not negative")
    return lr, beta1, beta2, eps, weight_decay, value_coef


def check_fit_batch(spec, n, labels_size=None, targets_size=None, alive_size=None):
    """The argument rules of ``bsk_fit_accumulate`` that need no device: n >= 1, value targets only with a value network, and
    every array given as long as n."""
    spec = _as_spec(spec)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1 or n > 2 ** 28:
        raise ValueError("n must be in 1..2^28, got %r" % (n,))
    if targets_size is not None and spec.value_hidden is None:
        raise ValueError("value targets given, but the policy has no value network")
    for what, size in (("labels", labels_size), ("value targets", targets_size), ("alive", alive_size)):
        if size is not None and int(size) != int(n):
            raise ValueError("%s: %d elements, got %d" % (what, n, size))
    return int(n)


def _fit_mask(n, labels, alive):
    """-> (labels int64 (n,), the samples that contribute: alive and a label in 0..2)"""
    labels = np.asarray(labels).reshape(-1).astype(np.int64)
    if labels.size != n:
        raise ValueError("labels: one per sample")
    on = (labels >= 0) & (labels <= 2)
    if alive is not None:
        alive = np.asarray(alive).reshape(-1)
        if alive.size != n:
            raise ValueError("alive: one byte per sample")
        on &= alive != 0
    return labels, on


def _fit_nets(spec, params, fp64):
    """-> in_scale, in_shift, the action network's [(W, b), ...], the value network's or None; float64 arrays under ``fp64`` - from
    ``params`` as it is, so that a float64 block is not rounded - float32 otherwise"""
    spec = _as_spec(spec)
    if not fp64:
        return unpack_params(spec, params)
    p = np.asarray(params, np.float64).reshape(-1)
    like = unpack_params(spec, np.zeros(p.size, np.float32))
    at, nets = 10, []
    for net in like[2:]:
        if net is None:
            nets.append(None)
            continue
        layers = []
        for W, b in net:
            layers.append((p[at:at + W.size].reshape(W.shape), p[at + W.size:at + W.size + b.size]))
            at += W.size + b.size
        nets.append(layers)
    return p[:5], p[5:10], nets[0], nets[1]


def _fit_forward(layers, activation, x, fp64):
    """One network with every layer kept -> [x, h_1, ..., output]: ``_forward32``'s chain, or float64 products under ``fp64``"""
    hs = [x]
    for li, (W, b) in enumerate(layers):
        h = hs[-1]
        if fp64:
            z = W @ h + b[:, None]
        else:
            z = np.broadcast_to(b[:, None], (W.shape[0], h.shape[1])).astype(np.float32)
            for k in range(W.shape[1]):
                z = fma32(W[:, k:k + 1], h[k:k + 1, :], z)
        if li + 1 < len(layers):
            with np.errstate(invalid="ignore"):
                z = np.tanh(z) if activation == "tanh" else np.where(z > 0, z, z.dtype.type(0))
        hs.append(z.astype(np.float64 if fp64 else np.float32))
    return hs


def _fit_inputs(scale, shift, obs, fp64):
    """(5, n) float64 observations -> x (5, n padded to whole blocks): a sample of the padding is an all-zero observation"""
    o = np.asarray(obs, np.float64).reshape(5, -1)
    n = o.shape[1]
    o32 = np.zeros((5, -(-n // FIT_BLOCK) * FIT_BLOCK), np.float32)
    o32[:, :n] = o.astype(np.float32)
    if fp64:
        return o32.astype(np.float64) * scale[:, None] + shift[:, None], n
    return fma32(o32, scale[:, None], shift[:, None]), n


def fit_dlogits_ref(spec, params, obs, labels, alive=None, value_targets=None, value_coef=0.0):
    """The output deltas in float64 from float64 logits (``mlp_ref(fp64=True)``'s, on ``params`` as given - a float64 block is not
    rounded) -> (dlogits (3, n), dvalue (n,) or None): p - onehot(label) and value_coef * (v - target), zeros where the sample does
    not contribute (alive == 0, or a label outside 0..2)."""
    spec = _as_spec(spec)
    scale, shift, a, v = _fit_nets(spec, params, True)
    x, n = _fit_inputs(scale, shift, obs, True)
    labels, on = _fit_mask(n, labels, alive)
    l = _fit_forward(a, spec.activation, x, True)[-1][:, :n]
    e = np.exp(l - l.max(axis=0))
    g = e / e.sum(axis=0)
    g[np.clip(labels, 0, 2), np.arange(n)] -= 1.0
    g = np.where(on, g, 0.0)
    if value_targets is None:
        return g, None
    if v is None:
        raise ValueError("value targets given, but the policy has no value network")
    val = _fit_forward(v, spec.value_activation, x, True)[-1][0, :n]
    return g, np.where(on, np.float64(value_coef) * (val - np.asarray(value_targets, np.float64).reshape(-1)), 0.0)


def fit_dlogits32_ref(spec, params, obs, labels, alive=None, value_targets=None, value_coef=0.0):
    """The output deltas as the kernel forms them, float32 -> (dlogits (3, n), dvalue (n,) or None): ``mlp_ref``'s logits and value,
    ``softmax_ref``'s m, e and s, p_i = e_i / s, g_i = p_i - (i == label); dvalue = float32(value_coef) * (v - float32(target));
    +0.0 where the sample does not contribute.  ``exp`` is the host's here and the device library's there, so these are the
    device's deltas to a bound, not bit for bit; everything behind them is (``fit_backward_ref``)."""
    spec = _as_spec(spec)
    o = np.asarray(obs, np.float64).reshape(5, -1)
    n = o.shape[1]
    labels, on = _fit_mask(n, labels, alive)
    l, val = mlp_ref(spec, params, o)
    _, e, s = softmax_ref(l)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = (e / s).astype(np.float32) - (np.arange(3)[:, None] == labels[None, :]).astype(np.float32)
    g = np.where(on, g, np.float32(0)).astype(np.float32)
    if value_targets is None:
        return g, None
    if val is None:
        raise ValueError("value targets given, but the policy has no value network")
    d = val - np.asarray(value_targets, np.float64).reshape(-1).astype(np.float32)
    return g, np.where(on, np.float32(value_coef) * d, np.float32(0)).astype(np.float32)


def fit_loss_ref(spec, params, obs, labels, alive=None, value_targets=None, value_coef=0.0):
    """The loss whose gradient the fit accumulates, float64 and on ``params`` as given: the SUM over the contributing samples of
    -log softmax(logits)[label] + value_coef * 0.5 * (v - target)**2.  For finite differences."""
    spec = _as_spec(spec)
    scale, shift, a, v = _fit_nets(spec, params, True)
    x, n = _fit_inputs(scale, shift, obs, True)
    labels, on = _fit_mask(n, labels, alive)
    l = _fit_forward(a, spec.activation, x, True)[-1][:, :n]
    d = l - l.max(axis=0)
    logp = d - np.log(np.exp(d).sum(axis=0))
    loss = -np.where(on, logp[np.clip(labels, 0, 2), np.arange(n)], 0.0).sum()
    if value_targets is not None:
        val = _fit_forward(v, spec.value_activation, x, True)[-1][0, :n]
        loss += np.float64(value_coef) * 0.5 * np.where(on, (val - np.asarray(value_targets, np.float64).reshape(-1)) ** 2, 0.0).sum()
    return float(loss)


def _fit_net_backward(layers, activation, hs, dz, fp64, out):
    """The backward sweep of one network from its output deltas ``dz`` (fan_out, n padded): per layer from the last the block
    gradients - GW[j][k] the sample-ascending ``fma32`` chain of d_z[j][s] * h[k][s] from +0.0, Gb[j] the sample-ascending sum of
    d_z[j][s] - appended to ``out`` as (W part, b part) per layer, LAST LAYER FIRST; then d_h[k] the j-ascending ``fma32`` chain of
    W[j][k] * d_z[j] from +0.0 and d_z of the layer below through the activation's derivative at h."""
    dt = np.float64 if fp64 else np.float32
    B = dz.shape[1] // FIT_BLOCK
    for li in range(len(layers) - 1, -1, -1):
        W, _ = layers[li]
        h = hs[li]
        dzb, hb = dz.reshape(dz.shape[0], B, FIT_BLOCK), h.reshape(h.shape[0], B, FIT_BLOCK)
        if fp64:
            gw = np.einsum("jbs,kbs->bjk", dzb, hb)
            gb = dzb.sum(axis=2).T
        else:
            gw = np.zeros((B, dz.shape[0], h.shape[0]), np.float32)
            gb = np.zeros((B, dz.shape[0]), np.float32)
            for s in range(FIT_BLOCK):
                gw = fma32(dzb[:, :, s].T[:, :, None], hb[:, :, s].T[:, None, :], gw)
                gb = gb + dzb[:, :, s].T
        out.append((gw.reshape(B, -1), gb))
        if li == 0:
            break
        if fp64:
            dh = W.T @ dz
        else:
            dh = np.zeros(h.shape, np.float32)
            for j in range(W.shape[0]):
                dh = fma32(W[j][:, None], dz[j][None, :], dh)
        if activation == "tanh":
            dz = (dh * (1.0 - h * h if fp64 else fma32(-h, h, np.float32(1.0)))).astype(dt)
        else:
            dz = np.where(h > 0, dh, dt(0))


def fit_backward_ref(spec, params, obs, dlogits, dvalue=None, fp64=False):
    """The block gradients of ``bsk_fit_accumulate`` from GIVEN output deltas -> G (n_blocks, n_params) in the C-ABI parameter
    order, the first ten columns zero; block b is the samples 64 b .. 64 b + 63, the last one filled with all-zero observations and
    zero deltas.  ``dlogits`` (3, n) float32 - the device's own ``d_dlogits``, taken as exact - and ``dvalue`` (n,) float32 or None
    (then the value network's columns are zero).  Default: the definition in float32, bit for bit the device's block gradients for
    ``relu`` networks (``tanh`` is the host's here).  ``fp64=True``: float64 throughout, on ``params`` and deltas as given."""
    spec = _as_spec(spec)
    dt = np.float64 if fp64 else np.float32
    scale, shift, a, v = _fit_nets(spec, params, fp64)
    x, n = _fit_inputs(scale, shift, obs, fp64)
    B = x.shape[1] // FIT_BLOCK
    cols = [np.zeros((B, 10), dt)]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for layers, act, delta, rows in ((a, spec.activation, dlogits, 3), (v, spec.value_activation, dvalue, 1)):
            if layers is None:
                continue
            if delta is None:
                cols.append(np.zeros((B, sum(W.size + b.size for W, b in layers)), dt))
                continue
            dz = np.zeros((rows, x.shape[1]), dt)
            dz[:, :n] = np.asarray(delta, dt).reshape(rows, n)
            out = []
            _fit_net_backward(layers, act, _fit_forward(layers, act, x, fp64), dz, fp64, out)
            for gw, gb in reversed(out):
                cols += [gw, gb]
    return np.concatenate(cols, axis=1)


def fit_accumulate_ref(A, count, G, contributing):
    """One ``bsk_fit_accumulate`` on the accumulators -> (A float64 (n_params,), count int): A_p = A_p + float64(G[b][p]) for b
    ascending, count + the contributing samples of the call.  ``A`` is not changed."""
    A = np.array(A, dtype=np.float64).reshape(-1)
    G = np.asarray(G)
    if G.ndim != 2 or G.shape[1] != A.size:
        raise ValueError("G: (n_blocks, n_params)")
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(G.shape[0]):
            A = A + G[b].astype(np.float64)
    return A, int(count) + int(contributing)


def fit_stats_ref(spec, params, obs, labels, alive=None, value_targets=None):
    """The diagnostics row of one accumulate -> float64 (4,), ``FIT_STATS_COLUMNS``: float32 logits, log-probability and value
    difference as the kernel forms them (``exp`` / ``log`` are the host's), widened and summed sample-ascending within a block, then
    block-ascending."""
    spec = _as_spec(spec)
    o = np.asarray(obs, np.float64).reshape(5, -1)
    n = o.shape[1]
    labels, on = _fit_mask(n, labels, alive)
    l, val = mlp_ref(spec, params, o)
    m, e, s = softmax_ref(l)
    with np.errstate(invalid="ignore", divide="ignore"):
        logp = (l[np.clip(labels, 0, 2), np.arange(n)] - m) - np.log(s)
    greedy, _ = act_ref(l)
    pad = -(-n // FIT_BLOCK) * FIT_BLOCK
    terms = np.zeros((2, pad), np.float64)
    terms[0, :n] = np.where(on, -logp.astype(np.float64), 0.0)
    if value_targets is not None:
        d = np.where(on, val - np.asarray(value_targets, np.float64).reshape(-1).astype(np.float32), np.float32(0)).astype(np.float64)
        terms[1, :n] = (d * d) * 0.5
    blocks = np.zeros((2, pad // FIT_BLOCK), np.float64)
    for s_ in range(FIT_BLOCK):
        blocks = blocks + terms[:, s_::FIT_BLOCK]
    row = np.zeros(2, np.float64)
    for b in range(blocks.shape[1]):
        row = row + blocks[:, b]
    return np.array([row[0], row[1], float((on & (greedy == labels)).sum()), float(on.sum())], np.float64)


FIT_GNORM_BLOCK = 1024                         # threads of the one workgroup under the gradient's global norm


def check_max_grad_norm(max_grad_norm):
    """The argument rule of ``bsk_fit_set_max_grad_norm`` -> the float: 0 (off) or finite and positive; ValueError where it returns
    BSK_EINVAL.  Needs no device."""
    max_grad_norm = float(max_grad_norm)
    if not np.isfinite(max_grad_norm) or max_grad_norm < 0.0:
        raise ValueError("max_grad_norm must be 0 (off) or finite and positive")
    return max_grad_norm


def fit_grad_norm_ref(A, count, n_update, max_norm):
    """The row ``bsk_fit_step`` leaves behind ``bsk_fit_grad_norm_device`` under ``bsk_fit_set_max_grad_norm(max_norm)`` ->
    (norm, scale) float64: g_q = A[10 + q] / count for q = 0 .. n_update - 11; thread i of 1 024 adds g_q * g_q for q = i, i + 1024,
    ... ascending from the first (+0.0 with none); each of the 16 waves joins its 64 in the fitness tree; the wave sums are added
    ascending; norm = sqrt(S), scale = max_norm / (norm if norm > max_norm else max_norm).  count == 0: (+0.0, 1.0)."""
    max_norm = np.float64(check_max_grad_norm(max_norm))
    if not max_norm > 0.0:
        raise ValueError("max_norm must be positive: with 0 the step forms no norm")
    if int(count) == 0:
        return np.float64(0.0), np.float64(1.0)
    A = np.asarray(A, np.float64).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        g = A[10:int(n_update)] / np.float64(int(count))
        gg = g * g
        s = np.zeros(FIT_GNORM_BLOCK, np.float64)
        s[:min(FIT_GNORM_BLOCK, gg.size)] = gg[:FIT_GNORM_BLOCK]
        for at in range(FIT_GNORM_BLOCK, gg.size, FIT_GNORM_BLOCK):
            chunk = gg[at:at + FIT_GNORM_BLOCK]
            s[:chunk.size] = s[:chunk.size] + chunk
        s = s.reshape(FIT_GNORM_BLOCK // 64, 64)
        for stride in _TREE:
            s[:, :stride] = s[:, :stride] + s[:, stride:2 * stride]
        S = s[0, 0]
        for w in range(1, s.shape[0]):
            S = S + s[w, 0]
        norm = np.sqrt(S)
        scale = max_norm / (norm if norm > max_norm else max_norm)
    return np.float64(norm), np.float64(scale)


def fit_step_ref(theta, m, v, beta_pow, steps, A, count, lr, beta1, beta2, eps, weight_decay, n_update=None, max_grad_norm=0.0):
    """What ``bsk_fit_step`` leaves -> (theta, m, v, beta_pow, steps, A, count), float64: nothing moves while count == 0; otherwise
    for p in 10 .. n_update - 1 (default: all; the action network's end when no accumulate since the last step carried value
    targets) g = A_p / count + weight_decay * theta_p, Adam's lines (``_adam_step_ref``, the evolution strategy's) and
    theta_p = theta_p - step: a descent.  beta_pow and steps move on; A and the count come back zero.  ``max_grad_norm`` > 0
    (``bsk_fit_set_max_grad_norm``): g = (A_p / count) * scale + weight_decay * theta_p with ``fit_grad_norm_ref``'s scale."""
    theta = np.array(theta, dtype=np.float64).reshape(-1)
    m, v = np.array(m, dtype=np.float64).reshape(-1), np.array(v, dtype=np.float64).reshape(-1)
    bp = np.array(beta_pow, dtype=np.float64).reshape(2)
    A = np.array(A, dtype=np.float64).reshape(-1)
    lr, b1, b2, eps, wd, _ = (np.float64(x) for x in check_fit(lr, beta1, beta2, eps, weight_decay, 0.0))
    max_grad_norm = check_max_grad_norm(max_grad_norm)
    hi = theta.size if n_update is None else int(n_update)
    if int(count) == 0:
        return theta, m, v, bp, int(steps), np.zeros_like(A), 0
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = theta[10:hi]
        if max_grad_norm > 0.0:
            g = (A[10:hi] / np.float64(int(count))) * fit_grad_norm_ref(A, count, hi, max_grad_norm)[1] + wd * t
        else:
            g = A[10:hi] / np.float64(int(count)) + wd * t
        m[10:hi], v[10:hi], step, bp = _adam_step_ref(m[10:hi], v[10:hi], bp, g, lr, b1, b2, eps)
        theta[10:hi] = t - step
    return theta, m, v, bp, int(steps) + 1, np.zeros_like(A), 0


# ---------------------------------------------------------------------------------------------------------------------------------
# Policy-gradient training on the fit (bsk_gae, bsk_fit_accumulate_pg; definition in include/bskgpu.h), restated

PG_STATS_COLUMNS = ("kl_sum", "entropy_sum", "clipped", "surrogate_sum")


def check_gae(n_steps, n_envs, stride, gamma, lam):
    """The argument rules of ``bsk_gae`` that need no device -> (n_steps, n_envs, stride, gamma, lam); ValueError where it returns
    BSK_EINVAL."""
    for what, x in (("n_steps", n_steps), ("n_envs", n_envs), ("stride", stride)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1:
            raise ValueError("%s must be an integer >= 1, got %r" % (what, x))
    if stride < n_envs:
        raise ValueError("stride must be >= n_envs")
    gamma, lam = float(gamma), float(lam)
    if not (0.0 <= gamma <= 1.0) or not (0.0 <= lam <= 1.0):
        raise ValueError("gamma and lam must be in [0, 1]")
    return int(n_steps), int(n_envs), int(stride), gamma, lam


def check_pg(clip, ent_coef, with_logp_old=True):
    """The argument rules ``bsk_fit_accumulate_pg`` adds to ``bsk_fit_accumulate``'s -> (clip, ent_coef) as floats; ValueError where
    it returns BSK_EINVAL: ``clip`` finite and inside (0, 1) when old log-probabilities are given (otherwise it is not read),
    ``ent_coef`` finite and not negative.  Needs no device."""
    clip, ent_coef = float(clip), float(ent_coef)
    if with_logp_old and not (np.isfinite(clip) and 0.0 < clip < 1.0):
        raise ValueError("clip must be inside (0, 1) when old log-probabilities are given")
    if not np.isfinite(ent_coef) or ent_coef < 0.0:
        raise ValueError("ent_coef must be finite and not negative")
    return clip, ent_coef


def check_pg_loop(n_steps, gamma, lam, clip, ent_coef, epochs, minibatches, substeps):
    """The argument rules of ``policy_fit.PolicyGradient`` that need neither env nor device -> the eight, checked."""
    for what, x in (("n_steps", n_steps), ("epochs", epochs), ("minibatches", minibatches), ("substeps", substeps)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1:
            raise ValueError("%s must be an integer >= 1, got %r" % (what, x))
    if n_steps % minibatches:
        raise ValueError("n_steps (%d) must be divisible by minibatches (%d)" % (n_steps, minibatches))
    _, _, _, gamma, lam = check_gae(n_steps, 1, 1, gamma, lam)
    clip, ent_coef = check_pg(clip, ent_coef)
    return int(n_steps), gamma, lam, clip, ent_coef, int(epochs), int(minibatches), int(substeps)


def gae_ref(reward, reason, value, last_value=None, gamma=0.99, lam=0.95):
    """``bsk_gae`` restated: ``reward`` float64, ``reason`` uint8 and ``value`` float32, each (T, N); ``last_value`` float32 (N,) or
    None (= 0) -> (adv float32 (T, N), ret float64 (T, N)).  Per env, float64, t descending, every operation rounded on its own:
    where reason == 0, carry = ((reward + gamma * next_v) - v) + (gamma * lam) * carry; elsewhere - EVERY reason, the time limit
    included - carry = reward - v; adv = float32(carry), ret = carry + v, next_v = v.  Bit for bit the device's."""
    reward = np.asarray(reward, np.float64)
    T, N = reward.shape
    reason = np.asarray(reason).reshape(T, N)
    value = np.asarray(value, np.float32).reshape(T, N)
    g = np.float64(gamma)
    gl = g * np.float64(lam)
    carry = np.zeros(N, np.float64)
    next_v = np.zeros(N, np.float64) if last_value is None else np.asarray(last_value, np.float32).reshape(N).astype(np.float64)
    adv, ret = np.empty((T, N), np.float32), np.empty((T, N), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(T - 1, -1, -1):
            v = value[t].astype(np.float64)
            carry = np.where(reason[t] == 0, ((reward[t] + g * next_v) - v) + gl * carry, reward[t] - v)
            adv[t] = carry.astype(np.float32)
            ret[t] = carry + v
            next_v = v
    return adv, ret


def adv_normalize_work_bytes(n):
    """``bsk_adv_normalize_work_bytes``: 8 * (4 + 3 * ceil(n / 64)), the device bytes ``bsk_adv_normalize`` needs for n columns."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError("n must be an integer >= 1, got %r" % (n,))
    return 8 * (4 + 3 * ((int(n) + 63) // 64))


def check_adv_normalize(rows, n, stride, eps):
    """The argument rules of ``bsk_adv_normalize`` that need no device -> (rows, n, stride, eps); ValueError where it returns
    BSK_EINVAL."""
    for what, x in (("rows", rows), ("n", n), ("stride", stride)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1:
            raise ValueError("%s must be an integer >= 1, got %r" % (what, x))
    if stride < n:
        raise ValueError("stride must be >= n")
    if int(rows) * int(stride) > 2 ** 31:
        raise ValueError("rows * stride must not exceed 2^31")
    eps = float(eps)
    if not np.isfinite(eps) or not (eps > 0.0):
        raise ValueError("eps must be finite and positive")
    return int(rows), int(n), int(stride), eps


def adv_normalize_ref(adv, alive=None, eps=1e-8):
    """``bsk_adv_normalize`` restated: ``adv`` float32 (rows, n), ``alive`` (rows, n) or None (every sample counts) ->
    (out float32 (rows, n), moments float64 (4,) = mean, sd, inv, N).  Float64, every operation rounded on its own: per column the
    rows ascending, a1 = a1 + x and a2 = a2 + x * x from +0.0 with +0.0 for a sample that does not count; per wave of 64 columns
    the fitness tree; the waves joined by ``obs_stats_totals_ref``'s rule; ``obs_moments_ref``'s mean and var; sd = sqrt(var),
    inv = 1 / (sd + eps); out = float32((x - mean) * inv), +0.0 where the sample does not count.  With N == 0 the moments are four
    +0.0 and ``out`` is ``adv`` as it was (the device writes nothing).  Bit for bit the device's."""
    adv = np.asarray(adv, np.float32)
    if adv.ndim != 2:
        raise ValueError("advantages: (rows, n)")
    rows, n = adv.shape
    rows, n, _, eps = check_adv_normalize(rows, n, n, eps)
    counts = np.ones((rows, n), bool) if alive is None else np.asarray(alive).reshape(rows, n) != 0
    W = (n + 63) // 64
    xd = np.zeros((rows, W * 64), np.float64)
    xd[:, :n] = np.where(counts, adv.astype(np.float64), 0.0)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        a = np.zeros((2, W * 64), np.float64)
        for t in range(rows):
            a[0] = a[0] + xd[t]
            a[1] = a[1] + xd[t] * xd[t]
        s = a.reshape(2, W, 64)
        for stride in _TREE:
            s[:, :, :stride] = s[:, :, :stride] + s[:, :, stride:2 * stride]
        part = np.zeros((W, 10), np.float64)
        part[:, 0], part[:, 5] = s[0, :, 0], s[1, :, 0]
        tot, _ = obs_stats_totals_ref((part, np.zeros(W, np.uint64)))
        N = int(counts.sum())
        if N == 0:
            return adv.copy(), np.zeros(4, np.float64)
        mean, var = (x[0] for x in obs_moments_ref(tot, N))
        sd = np.sqrt(var)
        inv = np.float64(1.0) / (sd + np.float64(eps))
        out = np.where(counts, ((adv.astype(np.float64) - mean) * inv).astype(np.float32), np.float32(0.0))
    return out.astype(np.float32), np.array([mean, sd, inv, np.float64(N)], np.float64)


def pg_clip_edges(clip):
    """-> (lo, hi) float32: 1.0f - (float)clip and 1.0f + (float)clip, as the host forms them once"""
    c = np.float32(clip)
    return np.float32(1.0) - c, np.float32(1.0) + c


def fit_pg_terms_ref(logits, actions, adv, logp_old=None, clip=0.2, ent_coef=0.0, on=None, fp64=False):
    """The policy-gradient output deltas and the per-sample terms of their diagnostics from GIVEN logits (3, n) -> dict ``g``
    (3, n), ``d``, ``r``, ``H``, ``clipped`` (bool), ``surrogate`` = A r, each (n,).  Default: float32 in the kernel's order
    (``softmax_ref``'s m, e and s; p_i = e_i / s; lp_i = (l_i - m) - log(s); ``fma32`` for the entropy term; ``exp`` and ``log`` are
    the host's).  ``fp64=True``: the same formulas in float64 on the logits as given, with the float32 clip edges widened.  Samples
    outside ``on`` (bool (n,), default all) get zero deltas; their other terms are still formed."""
    dt = np.float64 if fp64 else np.float32
    l = np.asarray(logits, dt).reshape(3, -1)
    n = l.shape[1]
    a = np.clip(np.asarray(actions).reshape(-1).astype(np.int64), 0, 2)
    A = np.asarray(adv, np.float32).reshape(-1).astype(dt)
    on = np.ones(n, bool) if on is None else np.asarray(on, bool).reshape(-1)
    lo, hi = (dt(x) for x in pg_clip_edges(clip))
    ec = dt(np.float32(ent_coef))
    pick = (a, np.arange(n))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore", under="ignore"):
        if fp64:
            z = l - l.max(axis=0)
            e = np.exp(z)
            s = e.sum(axis=0)
            p, lp = e / s, z - np.log(s)
        else:
            m, e, s = softmax_ref(l)
            p, lp = (e / s).astype(dt), ((l - m) - np.log(s)).astype(dt)
        H = -((p[0] * lp[0] + p[1] * lp[1]) + p[2] * lp[2])
        if logp_old is None:
            d, r, clipped = np.zeros(n, dt), np.ones(n, dt), np.zeros(n, bool)
        else:
            d = lp[pick] - np.asarray(logp_old, np.float32).reshape(-1).astype(dt)
            r = np.exp(d).astype(dt)
            clipped = ((A > 0) & (r > hi)) | ((A < 0) & (r < lo))
        onehot = (np.arange(3)[:, None] == a[None, :]).astype(dt)
        g = np.where(clipped | (A == 0), dt(0), (A * r) * (p - onehot)).astype(dt)
        if ec != 0:
            q = p * (lp + H)
            g = (g + ec * q) if fp64 else fma32(ec, q, g)
        g = np.where(on, g, dt(0)).astype(dt)
    return {"g": g, "d": d, "r": r, "H": H, "clipped": clipped, "surrogate": A * r if fp64 else A.astype(np.float64) * r.astype(np.float64)}


def fit_pg_dlogits32_ref(spec, params, obs, actions, adv, logp_old=None, clip=0.2, ent_coef=0.0, alive=None):
    """The policy-gradient output deltas as the kernel forms them, float32 (3, n): ``mlp_ref``'s logits through
    ``fit_pg_terms_ref``; +0.0 where the sample does not contribute (``_fit_mask`` with the action in the label's place).  With
    ``logp_old=None``, unit advantages and ``ent_coef=0`` these are ``fit_dlogits32_ref``'s bits for labels = actions."""
    spec = _as_spec(spec)
    o = np.asarray(obs, np.float64).reshape(5, -1)
    actions, on = _fit_mask(o.shape[1], actions, alive)
    return fit_pg_terms_ref(mlp_ref(spec, params, o)[0], actions, adv, logp_old, clip, ent_coef, on)["g"]


def fit_pg_dlogits_ref(spec, params, obs, actions, adv, logp_old=None, clip=0.2, ent_coef=0.0, alive=None, fp64=True):
    """The policy-gradient output deltas (3, n).  ``fp64=True``: float64 from float64 logits on ``params`` as given (a float64 block
    is not rounded), what ``fit_backward_ref(fp64=True)`` turns into the gradient of ``fit_pg_loss_ref``;  ``fp64=False``:
    ``fit_pg_dlogits32_ref``."""
    if not fp64:
        return fit_pg_dlogits32_ref(spec, params, obs, actions, adv, logp_old, clip, ent_coef, alive)
    spec = _as_spec(spec)
    scale, shift, a, _ = _fit_nets(spec, params, True)
    x, n = _fit_inputs(scale, shift, obs, True)
    actions, on = _fit_mask(n, actions, alive)
    l = _fit_forward(a, spec.activation, x, True)[-1][:, :n]
    return fit_pg_terms_ref(l, actions, adv, logp_old, clip, ent_coef, on, fp64=True)["g"]


def fit_pg_loss_ref(spec, params, obs, actions, adv, logp_old=None, clip=0.2, ent_coef=0.0, alive=None, value_targets=None,
                    value_coef=0.0):
    """The loss whose gradient ``bsk_fit_accumulate_pg`` accumulates, float64 and on ``params`` as given: the SUM over the
    contributing samples of -min(r A, clamp(r, lo, hi) A) - ent_coef H + value_coef * 0.5 * (v - target)**2, with
    r = exp(lp_a - logp_old); without ``logp_old`` the first term is -A lp_a, whose gradient is that of -r A at r = 1.  For finite
    differences: it has a kink where r crosses lo (A < 0) or hi (A > 0)."""
    spec = _as_spec(spec)
    scale, shift, a, v = _fit_nets(spec, params, True)
    x, n = _fit_inputs(scale, shift, obs, True)
    actions, on = _fit_mask(n, actions, alive)
    l = _fit_forward(a, spec.activation, x, True)[-1][:, :n]
    z = l - l.max(axis=0)
    lp = z - np.log(np.exp(z).sum(axis=0))
    lpa = lp[np.clip(actions, 0, 2), np.arange(n)]
    A = np.asarray(adv, np.float32).reshape(-1).astype(np.float64)
    if logp_old is None:
        per = -A * lpa
    else:
        lo, hi = (np.float64(e) for e in pg_clip_edges(clip))
        r = np.exp(lpa - np.asarray(logp_old, np.float32).reshape(-1).astype(np.float64))
        per = -np.minimum(r * A, np.clip(r, lo, hi) * A)
    H = -(np.exp(lp) * lp).sum(axis=0)
    loss = np.where(on, per - np.float64(np.float32(ent_coef)) * H, 0.0).sum()
    if value_targets is not None:
        val = _fit_forward(v, spec.value_activation, x, True)[-1][0, :n]
        loss += np.float64(value_coef) * 0.5 * np.where(on, (val - np.asarray(value_targets, np.float64).reshape(-1)) ** 2, 0.0).sum()
    return float(loss)


def fit_pg_stats_ref(spec, params, obs, actions, adv, logp_old=None, clip=0.2, alive=None):
    """The policy-gradient row of one ``bsk_fit_accumulate_pg`` -> float64 (4,), ``PG_STATS_COLUMNS``: the float32 terms of
    ``fit_pg_terms_ref`` on ``mlp_ref``'s logits, widened and summed sample-ascending within a block, then block-ascending;
    contributing samples only."""
    spec = _as_spec(spec)
    o = np.asarray(obs, np.float64).reshape(5, -1)
    n = o.shape[1]
    actions, on = _fit_mask(n, actions, alive)
    t = fit_pg_terms_ref(mlp_ref(spec, params, o)[0], actions, adv, logp_old, clip, 0.0, on)
    pad = -(-n // FIT_BLOCK) * FIT_BLOCK
    terms = np.zeros((4, pad), np.float64)
    terms[0, :n] = np.where(on, -t["d"].astype(np.float64), 0.0)
    terms[1, :n] = np.where(on, t["H"].astype(np.float64), 0.0)
    terms[2, :n] = np.where(on & t["clipped"], 1.0, 0.0)
    terms[3, :n] = np.where(on, t["surrogate"], 0.0)
    blocks = np.zeros((4, pad // FIT_BLOCK), np.float64)
    for s_ in range(FIT_BLOCK):
        blocks = blocks + terms[:, s_::FIT_BLOCK]
    row = np.zeros(4, np.float64)
    for b in range(blocks.shape[1]):
        row = row + blocks[:, b]
    return row


# ---------------------------------------------------------------------------------------------------------------------------------
# Shuffled minibatches and the clipped value loss (bsk_pg_gather, bsk_fit_accumulate_ppo; definition in include/bskgpu.h), restated

PG_SHUFFLE_ROUNDS = 8
PG_SHUFFLE_TAG = 0x50475348                    # "PGSH": the third counter word of the key draws
VCLIP_STATS_COLUMNS = ("value_clipped", "value_loss_unclipped_sum")


def pg_shuffle_keys_ref(seed, epoch):
    """The eight round keys of the permutation of ``{seed, epoch}`` -> uint64 (8,) holding 32-bit words: two draws of
    ``philox4x32_10`` with counter (epoch_lo, epoch_hi, PG_SHUFFLE_TAG, i) under key (seed_lo, seed_hi), i = 0, 1.  ``epoch`` may be
    an array of E epochs: -> (8, E), a column per epoch."""
    seed = np.uint64(int(seed) & (2 ** 64 - 1))
    scalar = np.ndim(epoch) == 0
    epoch = np.array([int(e) & (2 ** 64 - 1) for e in np.atleast_1d(epoch)], np.uint64)
    i = np.arange(2, dtype=np.uint64)[:, None]
    w = philox4x32_10(epoch & _MASK32, epoch >> _SH32, np.uint64(PG_SHUFFLE_TAG), i, seed & _MASK32, seed >> _SH32)
    keys = np.stack([np.broadcast_to(x, (2, epoch.size)) for x in w], axis=1).reshape(8, epoch.size).astype(np.uint64)
    return keys[:, 0] if scalar else keys


def _pg_fmix(h):
    """murmur3's finaliser on uint64 arrays that hold 32-bit words"""
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _MASK32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _MASK32
    return h ^ (h >> np.uint64(16))


def pg_perm_keys_ref(keys, N, q):
    """perm(q) under GIVEN round keys (8 words): the unbalanced Feistel network over 2^b values, b = max(2, bit_length(N - 1)),
    walked until it lands below N - every element for as many trips as IT needs, no cap -> int64, the shape of ``q``.  ``keys``
    (8, E) with ``q`` (E, ...): row e of ``q`` under column e of the keys."""
    N = int(N)
    if not 1 <= N < 2 ** 31:
        raise ValueError("N must be in 1 .. 2^31 - 1, got %r" % (N,))
    q = np.asarray(q, np.int64)
    if q.size and (q.min() < 0 or q.max() >= N):
        raise ValueError("q must lie in 0 .. N - 1")
    k = np.asarray(keys, np.uint64) & _MASK32
    if k.ndim == 1:
        k = np.broadcast_to(k.reshape(PG_SHUFFLE_ROUNDS, 1), (PG_SHUFFLE_ROUNDS, q.size))
    else:
        if q.ndim < 1 or k.shape != (PG_SHUFFLE_ROUNDS, q.shape[0]):
            raise ValueError("keys (8, E) need q (E, ...)")
        k = np.repeat(k, q.size // max(q.shape[0], 1), axis=1)
    b = max(2, (N - 1).bit_length())
    a = b >> 1
    c = b - a
    mask = {a: np.uint64((1 << a) - 1), c: np.uint64((1 << c) - 1)}
    x = q.reshape(-1).astype(np.uint64)
    todo = np.arange(x.size)
    while todo.size:
        v, kr = x[todo], k[:, todo]
        L, R = v >> np.uint64(c), v & mask[c]
        wl, wr = a, c
        for r in range(PG_SHUFFLE_ROUNDS):
            F = _pg_fmix(R ^ kr[r]) & mask[wl]
            L, R = R, L ^ F
            wl, wr = wr, wl
        v = (L << np.uint64(wr)) | R
        x[todo] = v
        todo = todo[v >= np.uint64(N)]
    return x.astype(np.int64).reshape(q.shape)


def pg_perm_ref(seed, epoch, N, q):
    """``bsk_pg_gather``'s permutation of [0, N) under the state words ``{seed, epoch}`` at the positions ``q`` -> int64, the shape
    of ``q``.  Integer arithmetic alone: bit for bit the device's (csrc/bsk_shuffle.hpp)."""
    return pg_perm_keys_ref(pg_shuffle_keys_ref(seed, epoch), N, q)


def pg_gather_ref(state, n_envs, q0, m, obs=None, **hist):
    """``bsk_pg_gather`` restated: a ``take`` by ``pg_perm_ref``.  ``state``: (seed, epoch) or None (the identity); ``obs``
    (n_steps, 5, n_envs) or None; every other history (n_steps, n_envs) by keyword -> dict: ``index`` int64 (m,), ``obs`` (5, m)
    and each history given (m,), in its own dtype."""
    arrays = {k: np.asarray(v) for k, v in hist.items() if v is not None}
    obs = None if obs is None else np.asarray(obs)
    first = obs if obs is not None else next(iter(arrays.values()))
    N = first.shape[0] * int(n_envs)
    q = int(q0) + np.arange(int(m), dtype=np.int64)
    if q0 < 0 or m < 1 or q0 + m > N:
        raise ValueError("the window q0 .. q0 + m - 1 must lie inside 0 .. N - 1")
    s = q if state is None else pg_perm_ref(state[0], state[1], N, q)
    t, j = s // int(n_envs), s % int(n_envs)
    out = {"index": s}
    if obs is not None:
        out["obs"] = np.ascontiguousarray(obs[t, :, j].T)
    for k, v in arrays.items():
        out[k] = v[t, j]
    return out


def fit_value_delta_ref(v, R, value_old=None, clip_vf=None, value_coef=0.5):
    """The value network's output delta and loss term of ``bsk_fit_accumulate_ppo`` per contributing sample -> (delta float32,
    term float64, clipped bool), each (n,).  ``v`` the network's float32 outputs, ``R`` the targets (rounded to float32 here, as
    the kernel rounds them), ``value_old`` float32 or None.  Float32, every operation rounded on its own: d = v - R; without
    ``value_old``, or with -cv <= v - value_old <= cv: delta = value_coef * d, term = d d / 2 (the product and the half in
    float64); else vc = value_old +- cv, d2 = vc - R, and where d2 d2 > d d: delta = +0.0, term = d2 d2 / 2, clipped.  A tie is
    the unclipped branch's.  Bit for bit the device's."""
    v = np.asarray(v, np.float32).reshape(-1)
    R = np.asarray(R).reshape(-1).astype(np.float32)
    vc32 = np.float32(value_coef)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        d = (v - R).astype(np.float32)
        delta = (vc32 * d).astype(np.float32)
        term = (d.astype(np.float64) * d.astype(np.float64)) * 0.5
        clipped = np.zeros(v.size, bool)
        if value_old is not None:
            cv = np.float32(clip_vf)
            vo = np.asarray(value_old, np.float32).reshape(-1)
            dv = (v - vo).astype(np.float32)
            outside = ~((-cv <= dv) & (dv <= cv))
            vcl = (vo + np.where(dv > 0, cv, -cv).astype(np.float32)).astype(np.float32)
            d2 = (vcl - R).astype(np.float32)
            clipped = outside & ((d2 * d2).astype(np.float32) > (d * d).astype(np.float32))
            delta = np.where(clipped, np.float32(0.0), delta).astype(np.float32)
            term = np.where(clipped, (d2.astype(np.float64) * d2.astype(np.float64)) * 0.5, term)
    return delta, term, clipped


def check_pg_shuffle(shuffle=False, seed=0, cliprange_vf=None, n_steps=1, minibatches=1, n_envs=1):
    """The argument rules ``PolicyGradient`` adds for shuffled minibatches and the clipped value loss, beside ``check_pg_loop``'s
    -> (shuffle, seed, cliprange_vf): ``shuffle`` a bool, ``seed`` an integer in 0 .. 2^64 - 1, ``cliprange_vf`` None (the plain
    squared error) or finite and positive - where ``bsk_fit_accumulate_ppo`` returns BSK_EINVAL otherwise -, and with ``shuffle``
    n_steps * n_envs below 2^31, ``bsk_pg_gather``'s bound.  Needs no device."""
    if not isinstance(shuffle, (bool, np.bool_)):
        raise ValueError("shuffle must be a bool, got %r" % (shuffle,))
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must be an integer in 0 .. 2^64 - 1, got %r" % (seed,))
    if cliprange_vf is not None:
        if isinstance(cliprange_vf, bool):
            raise ValueError("cliprange_vf must be None or a positive number")
        cliprange_vf = float(cliprange_vf)
        if not np.isfinite(cliprange_vf) or not (cliprange_vf > 0.0):
            raise ValueError("cliprange_vf must be None or finite and positive")
    for what, x in (("n_steps", n_steps), ("minibatches", minibatches), ("n_envs", n_envs)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1:
            raise ValueError("%s must be an integer >= 1, got %r" % (what, x))
    if shuffle and int(n_steps) * int(n_envs) >= 2 ** 31:
        raise ValueError("shuffle: n_steps * n_envs must be below 2^31")
    return bool(shuffle), int(seed), cliprange_vf


def check_pg_gather(n_steps, n_envs, stride, q0, m, out_stride):
    """The argument rules of ``bsk_pg_gather`` that need no device -> the six as ints; ValueError where it returns BSK_EINVAL."""
    for what, x, least in (("n_steps", n_steps, 1), ("n_envs", n_envs, 1), ("stride", stride, 1), ("q0", q0, 0), ("m", m, 1),
                           ("out_stride", out_stride, 0)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < least:
            raise ValueError("%s must be an integer >= %d, got %r" % (what, least, x))
    n_steps, n_envs, stride, q0, m, out_stride = (int(x) for x in (n_steps, n_envs, stride, q0, m, out_stride))
    if n_steps * n_envs >= 2 ** 31:
        raise ValueError("n_steps * n_envs must be below 2^31")
    if stride < n_envs:
        raise ValueError("stride must be >= n_envs")
    if q0 + m > n_steps * n_envs:
        raise ValueError("the window q0 .. q0 + m - 1 must lie inside 0 .. n_steps * n_envs - 1")
    return n_steps, n_envs, stride, q0, m, out_stride


# ---------------------------------------------------------------------------------------------------------------------------------
# A training log for the policy-gradient loop (bsk_pg_episodes, bsk_pg_log_update, bsk_pg_log_advance; definition in
# include/bskgpu.h, kernels in csrc/bsk_pglog.hip), restated

PG_LOG_COLUMNS = ("episodes", "return_sum", "return_sum_sq", "return_min", "return_max", "len_sum",
                  "end_length", "end_wheels", "end_battery", "end_orbit", "act_0", "act_1", "act_2", "reward_sum",
                  "explained_variance", "value_err_sum_sq") + PG_STATS_COLUMNS + FIT_STATS_COLUMNS + ("grad_norm_sum", "grad_clipped")
PG_LOG_COLS = len(PG_LOG_COLUMNS)              # BSK_PG_LOG_COLS
PG_EP_WORDS = 19                               # words of one wave's partial row: 7 sums, 2 extremes, 10 counts
PG_EP_SUMS = ("s_R", "s_R2", "s_rew", "s_y", "s_y2", "s_e", "s_e2")
PG_EP_COUNTS = ("n_ep", "len_sum", "end_length", "end_wheels", "end_battery", "end_orbit", "act_0", "act_1", "act_2", "samples")


def pg_episodes_work_bytes(n_envs):
    """``bsk_pg_episodes_work_bytes``: 8 * 19 * ceil(n_envs / 64), the device bytes ``bsk_pg_episodes`` needs for its partial rows."""
    if isinstance(n_envs, bool) or not isinstance(n_envs, (int, np.integer)) or n_envs < 1:
        raise ValueError("n_envs must be an integer >= 1, got %r" % (n_envs,))
    return 8 * PG_EP_WORDS * ((int(n_envs) + 63) // 64)


def check_pg_episodes(n_steps, n_envs, stride, capacity, with_value=False, with_ret=False):
    """The argument rules of ``bsk_pg_episodes`` that need no device -> (n_steps, n_envs, stride, capacity); ValueError where it
    returns BSK_EINVAL: each an integer >= 1, stride >= n_envs, n_steps * stride <= 2^31, value and return histories both or
    neither."""
    for what, x in (("n_steps", n_steps), ("n_envs", n_envs), ("stride", stride), ("capacity", capacity)):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1:
            raise ValueError("%s must be an integer >= 1, got %r" % (what, x))
    if stride < n_envs:
        raise ValueError("stride must be >= n_envs")
    if int(n_steps) * int(stride) > 2 ** 31:
        raise ValueError("n_steps * stride must not exceed 2^31")
    if bool(with_value) != bool(with_ret):
        raise ValueError("the value and the return histories are given together or not at all")
    return int(n_steps), int(n_envs), int(stride), int(capacity)


def check_pg_log(n_rows, capacity, n_norms=None):
    """The argument rules of ``bsk_pg_log_update`` (and, with n_rows = 1, of ``bsk_pg_log_advance``) that need no device ->
    (n_rows, capacity, n_norms): n_rows and capacity integers >= 1; ``n_norms`` None (no norms) or an integer >= 1."""
    for what, x in (("n_rows", n_rows), ("capacity", capacity)) + ((("n_norms", n_norms),) if n_norms is not None else ()):
        if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or x < 1:
            raise ValueError("%s must be an integer >= 1, got %r" % (what, x))
    return int(n_rows), int(capacity), None if n_norms is None else int(n_norms)


def _pg_episode_state(state, n):
    if state is None:
        return np.zeros(n, np.float64), np.zeros(n, np.int32)
    R, L = np.array(state[0], dtype=np.float64).reshape(-1), np.array(state[1], dtype=np.int32).reshape(-1)
    if R.shape != (n,) or L.shape != (n,):
        raise ValueError("state: (ep_return float64 (%d,), ep_len int32 (%d,))" % (n, n))
    return R, L


def pg_episodes_walk_ref(reward, reason, action=None, value=None, ret=None, state=None):
    """The per-column walk of ``bsk_pg_episodes`` (csrc/bsk_pglog.hpp: pg_episode_walk), every column at once -> (sums float64
    (7, N) in ``PG_EP_SUMS``' order, mn float64 (N,), mx float64 (N,), counts int64 (10, N) in ``PG_EP_COUNTS``' order,
    (ep_return float64 (N,), ep_len int32 (N,))): what each lane holds in front of the trees, and the state it writes back.
    ``reward`` float64, ``reason`` uint8, ``action`` int32 or None, ``value`` float32 and ``ret`` float64 (both or neither), each
    (T, N); ``state``: the carried (ep_return, ep_len) or None (zeros: fresh envs).  Rows ascending, every operation rounded on its
    own."""
    reward = np.asarray(reward, np.float64)
    if reward.ndim != 2 or reward.shape[0] < 1 or reward.shape[1] < 1:
        raise ValueError("reward: (n_steps, n_envs)")
    T, N = reward.shape
    check_pg_episodes(T, N, N, 1, value is not None, ret is not None)
    reason = np.asarray(reason).reshape(T, N).astype(np.uint8)
    action = None if action is None else np.asarray(action, np.int32).reshape(T, N)
    if value is not None:
        value, ret = np.asarray(value, np.float32).reshape(T, N), np.asarray(ret, np.float64).reshape(T, N)
    R, L = _pg_episode_state(state, N)
    L = L.astype(np.int64)
    s = np.zeros((7, N), np.float64)
    mn, mx = np.full(N, np.nan, np.float64), np.full(N, np.nan, np.float64)
    k = np.zeros((10, N), np.int64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for t in range(T):
            R = R + reward[t]
            L = L + 1
            s[2] = s[2] + reward[t]
            k[9] += 1
            if action is not None:
                for a in range(3):
                    k[6 + a] += action[t] == a
            if value is not None:
                y = ret[t]
                e = y - value[t].astype(np.float64)
                s[3] = s[3] + y
                s[4] = s[4] + y * y
                s[5] = s[5] + e
                s[6] = s[6] + e * e
            q = reason[t] != 0
            s[0] = np.where(q, s[0] + R, s[0])
            s[1] = np.where(q, s[1] + R * R, s[1])
            mn = np.where(q, _extreme_pick(mn, R, False), mn)
            mx = np.where(q, _extreme_pick(mx, R, True), mx)
            k[0] += q
            k[1] += np.where(q, L, 0)
            for b in range(4):
                k[2 + b] += q & ((reason[t] & (1 << b)) != 0)
            R = np.where(q, np.float64(0.0), R)
            L = np.where(q, 0, L)
    return s, mn, mx, k, (R, L.astype(np.int32))


def pg_episodes_ref(reward, reason, action=None, value=None, ret=None, state=None):
    """``bsk_pg_episodes`` restated -> (row float64 (16,): columns 0 .. 15 of ``PG_LOG_COLUMNS``, (ep_return float64 (N,), ep_len
    int32 (N,)): the new state).  ``pg_episodes_walk_ref`` per column; per wave of 64 columns (lanes at and above N bring +0.0, NaN
    and 0) the seven sums through the fitness tree and the two extremes through it under their own rule; the waves joined by
    ``obs_stats_totals_ref``'s rule - lane l the partials l, l + 64, ... ascending from the first, then the tree; the counts as
    integers, converted once; the explained variance 1 - var_e / var_y out of ``obs_moments_ref`` on (S_y, S_y2, N) and (S_e, S_e2, N),
    NaN when var_y == 0 or without ``value`` / ``ret``.  Bit for bit the device's."""
    s, mn, mx, k, new_state = pg_episodes_walk_ref(reward, reason, action, value, ret, state)
    N = s.shape[1]
    W = (N + 63) // 64
    lanes = np.zeros((7, W * 64), np.float64)
    lanes[:, :N] = s
    ext = np.full((2, W * 64), np.nan, np.float64)
    ext[0, :N], ext[1, :N] = mn, mx
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        tree = lanes.reshape(7, W, 64)
        for stride in _TREE:
            tree[:, :, :stride] = tree[:, :, :stride] + tree[:, :, stride:2 * stride]
        part = np.zeros((W, 10), np.float64)
        part[:, :7] = tree[:, :, 0].T
        tot, _ = obs_stats_totals_ref((part, np.zeros(W, np.uint64)))
        lo = _extreme_lanes_then_tree(_extreme_lanes_then_tree(ext[0].reshape(W, 64), False), False)
        hi = _extreme_lanes_then_tree(_extreme_lanes_then_tree(ext[1].reshape(W, 64), True), True)
        n = k.sum(axis=1)
        row = np.zeros(16, np.float64)
        row[0], row[1], row[2], row[3], row[4], row[5] = np.float64(n[0]), tot[0], tot[1], lo, hi, np.float64(n[1])
        row[6:13] = n[2:9].astype(np.float64)
        row[13] = tot[2]
        row[14] = np.nan
        if value is not None:
            _, var = obs_moments_ref(np.array([tot[3], tot[5], 0, 0, 0, tot[4], tot[6], 0, 0, 0], np.float64), int(n[9]))
            if var[0] != 0.0:
                row[14] = np.float64(1.0) - var[1] / var[0]
        row[15] = tot[6]
    return row, new_state


def pg_log_update_ref(diag, norms=None):
    """``bsk_pg_log_update`` restated -> float64 (10,): columns 16 .. 25 of ``PG_LOG_COLUMNS``.  ``diag`` float64 (n_rows, 8): each
    column summed, rows ascending FROM the first; ``norms`` float64 (n_norms, 2) = {norm, scale} rows or None: the norms summed the
    same way and the rows with scale < 1.0 counted; +0.0 and 0 without."""
    diag = np.asarray(diag, np.float64)
    if diag.ndim != 2 or diag.shape[1] != 8:
        raise ValueError("diag: (n_rows, 8)")
    check_pg_log(diag.shape[0], 1, None if norms is None else np.asarray(norms).shape[0])
    out = np.zeros(10, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = diag[0].copy()
        for r in range(1, diag.shape[0]):
            s = s + diag[r]
        out[:8] = s
        if norms is not None:
            norms = np.asarray(norms, np.float64)
            if norms.ndim != 2 or norms.shape[1] != 2:
                raise ValueError("norms: (n_norms, 2)")
            t = norms[0, 0]
            for r in range(1, norms.shape[0]):
                t = t + norms[r, 0]
            out[8], out[9] = t, np.float64(int((norms[:, 1] < 1.0).sum()))
    return out


def pg_log_table_ref(gen, rows):
    """The ring as the device holds it -> ``training_log``'s (iterations uint64 (k,), rows float64 (k, 26)) over the slots that have
    been written (``gen`` is not all ones), oldest first."""
    gen = np.asarray(gen, np.uint64).reshape(-1)
    rows = np.asarray(rows, np.float64).reshape(gen.size, PG_LOG_COLS)
    valid = np.flatnonzero(gen != np.uint64(ES_LOG_EMPTY))
    valid = valid[np.argsort(gen[valid], kind="stable")]
    return gen[valid].copy(), rows[valid].copy()


# ---------------------------------------------------------------------------------------------------------------------------------
# Rewards scaled by the running deviation of the discounted return (bsk_reward_norm; definition in include/bskgpu.h, kernels in
# csrc/bsk_rewnorm.hip), restated

REWARD_NORM_STATE_WORDS = 8                    # BSK_REWARD_NORM_STATE_WORDS
REWARD_NORM_STATE_FIELDS = ("sum", "sum_sq", "count", "mean", "var", "sd", "calls", "zero")


def reward_norm_work_bytes(n):
    """``bsk_reward_norm_work_bytes``: 8 * 3 * ceil(n / 64), the device bytes ``bsk_reward_norm`` needs for its partial rows."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError("n must be an integer >= 1, got %r" % (n,))
    return 8 * 3 * ((int(n) + 63) // 64)


def check_reward_norm(n_steps, n_envs, stride, gamma, eps, clip):
    """The argument rules of ``bsk_reward_norm`` that need no device -> (n_steps, n_envs, stride, gamma, eps, clip); ValueError
    where it returns BSK_EINVAL: the size rules of ``check_pg_episodes``; gamma in [0, 1]; eps finite and not negative; clip
    greater than 0 (+inf is allowed: nothing is then clipped) and not a NaN."""
    n_steps, n_envs, stride, _ = check_pg_episodes(n_steps, n_envs, stride, 1)
    gamma, eps, clip = float(gamma), float(eps), float(clip)
    if not (0.0 <= gamma <= 1.0):
        raise ValueError("gamma must be in [0, 1]")
    if not np.isfinite(eps) or eps < 0.0:
        raise ValueError("eps must be finite and not negative")
    if not (clip > 0.0):
        raise ValueError("clip must be greater than 0")
    return n_steps, n_envs, stride, gamma, eps, clip


def reward_norm_state_words(state=None):
    """The eight state words as uint64 (8,), a copy: None -> all zero, a fresh state.  Words 0, 1, 3, 4 and 5 are the bits of float64
    numbers (``.view(numpy.float64)``), words 2 and 6 integers (``REWARD_NORM_STATE_FIELDS``)."""
    if state is None:
        return np.zeros(REWARD_NORM_STATE_WORDS, np.uint64)
    words = np.array(state, copy=True)
    if words.dtype != np.uint64 or words.shape != (REWARD_NORM_STATE_WORDS,):
        raise ValueError("state: uint64 (%d,), the words as the device holds them" % REWARD_NORM_STATE_WORDS)
    return words


def reward_norm_divisor(state):
    """What the apply divides by: sd when something has been counted, 1.0 on a fresh state."""
    words = reward_norm_state_words(state)
    return np.float64(words.view(np.float64)[5]) if int(words[2]) != 0 else np.float64(1.0)


def reward_norm_walk_ref(reward, reason, gamma, ret_run=None):
    """The per-column walk of ``bsk_reward_norm`` (csrc/bsk_rewnorm.hpp: reward_norm_walk), every column at once -> (a1 float64 (N,),
    a2 float64 (N,), k int64 (N,), ret_run float64 (N,)): what each lane holds in front of the trees, and the running return it
    writes back.  ``reward`` float64 and ``reason`` uint8, each (T, N); ``ret_run``: the carried returns or None (zeros: fresh
    envs).  Rows ascending, every operation rounded on its own: R = gamma * R + reward; a1 = a1 + R; a2 = a2 + R * R; k += 1; then
    R = +0.0 where the reason byte is not zero."""
    reward = np.asarray(reward, np.float64)
    if reward.ndim != 2 or reward.shape[0] < 1 or reward.shape[1] < 1:
        raise ValueError("reward: (n_steps, n_envs)")
    T, N = reward.shape
    _, _, _, gamma, _, _ = check_reward_norm(T, N, N, gamma, 0.0, 1.0)
    reason = np.asarray(reason).reshape(T, N).astype(np.uint8)
    R = np.zeros(N, np.float64) if ret_run is None else np.array(ret_run, dtype=np.float64).reshape(-1)
    if R.shape != (N,):
        raise ValueError("ret_run: float64 (%d,)" % N)
    g = np.float64(gamma)
    a1, a2, k = np.zeros(N, np.float64), np.zeros(N, np.float64), np.zeros(N, np.int64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for t in range(T):
            R = g * R + reward[t]
            a1 = a1 + R
            a2 = a2 + R * R
            k += 1
            R = np.where(reason[t] != 0, np.float64(0.0), R)
    return a1, a2, k, R


def reward_norm_ref(reward, reason, gamma, eps, clip, update, state=None, ret_run=None, with_work=False):
    """``bsk_reward_norm`` restated -> (out float64 (T, N), state uint64 (8,), ret_run float64 (N,)) and, ``with_work``, the partial
    rows uint64 (W, 3) as the device leaves them (None without ``update``).  ``state``: the eight words carried in
    (``reward_norm_state_words``; None: fresh) and ``ret_run`` the running returns (None: zeros); neither is changed.  With
    ``update``: ``reward_norm_walk_ref`` per column; per wave of 64 columns (lanes at and above N bring +0.0 and 0) the two sums
    through the fitness tree; the waves joined by ``obs_stats_totals_ref``'s rule; sum, sum_sq and count added to, calls += 1;
    ``obs_moments_ref``'s mean and var; sd = sqrt(var + eps).  Always: d = sd where count != 0 and 1.0 otherwise - behind the
    update, so the WHOLE rollout is divided by the deviation that already holds it -, y = reward / d, clipped to [-clip, clip], a NaN
    passing through.  Bit for bit the device's."""
    reward = np.asarray(reward, np.float64)
    if reward.ndim != 2 or reward.shape[0] < 1 or reward.shape[1] < 1:
        raise ValueError("reward: (n_steps, n_envs)")
    T, N = reward.shape
    _, _, _, gamma, eps, clip = check_reward_norm(T, N, N, gamma, eps, clip)
    words = reward_norm_state_words(state)
    R = np.zeros(N, np.float64) if ret_run is None else np.array(ret_run, dtype=np.float64).reshape(-1)
    if R.shape != (N,):
        raise ValueError("ret_run: float64 (%d,)" % N)
    work = None
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        if update:
            a1, a2, k, R = reward_norm_walk_ref(reward, reason, gamma, R)
            W = (N + 63) // 64
            lanes = np.zeros((2, W * 64), np.float64)
            lanes[0, :N], lanes[1, :N] = a1, a2
            tree = lanes.reshape(2, W, 64)
            for stride in _TREE:
                tree[:, :, :stride] = tree[:, :, :stride] + tree[:, :, stride:2 * stride]
            counts = np.zeros(W * 64, np.int64)
            counts[:N] = k
            counts = counts.reshape(W, 64).sum(axis=1)
            work = np.empty((W, 3), np.uint64)
            work[:, 0], work[:, 1] = tree[0, :, 0].view(np.uint64), tree[1, :, 0].view(np.uint64)
            work[:, 2] = counts.astype(np.uint64)
            part = np.zeros((W, 10), np.float64)
            part[:, 0], part[:, 5] = tree[0, :, 0], tree[1, :, 0]
            tot, _ = obs_stats_totals_ref((part, np.zeros(W, np.uint64)))
            f = words.view(np.float64)
            total = np.array([f[0] + tot[0], 0, 0, 0, 0, f[1] + tot[5], 0, 0, 0, 0], np.float64)
            count = (int(words[2]) + int(counts.sum())) % 2 ** 64
            mean, var = (x[0] for x in obs_moments_ref(total, count))
            f[0], f[1], f[3], f[4], f[5] = total[0], total[5], mean, var, np.sqrt(var + np.float64(eps))
            words[2], words[6], words[7] = count, (int(words[6]) + 1) % 2 ** 64, 0
        d = reward_norm_divisor(words)
        y = reward / d
        c = np.float64(clip)
        out = np.where(y > c, c, np.where(y < -c, -c, y))
    return (out, words, R, work) if with_work else (out, words, R)


# ---------------------------------------------------------------------------------------------------------------------------------
# Schedules of lr, clip, clip_vf and ent_coef and a KL stop per update (bsk_fit_set_schedule, bsk_fit_schedule_begin,
# bsk_fit_kl_gate, bsk_fit_schedule_end; definition in include/bskgpu.h, kernels in csrc/bsk_pgsched.hip), restated

SCHED_WORDS = 8                                # BSK_FIT_SCHEDULE_WORDS
SCHED_STATE_FIELDS = ("lr", "clip", "clip_vf", "ent_coef", "iteration", "gate", "steps_skipped", "kl_at_stop")
SCHED_LOG_COLUMNS = ("iteration", "lr", "clip", "clip_vf", "ent_coef", "steps_skipped", "kl_at_stop", "stopped")


def _sched_pair(what, x):
    try:
        a, b = x
        if isinstance(a, bool) or isinstance(b, bool):
            raise TypeError
        return float(a), float(b)
    except (TypeError, ValueError):
        raise ValueError("%s: a pair (a, b) of numbers, got %r" % (what, x)) from None


def check_pg_schedule(total, lr, clip, clip_vf, ent_coef, kl_stop=0.0):
    """The argument rules of ``bsk_fit_set_schedule`` -> (total, lr, clip, clip_vf, ent_coef, kl_stop), the four pairs as tuples of
    floats; ValueError where it returns BSK_EINVAL.  Both ends of a pair obey the rule of the argument they stand in for: ``lr``
    finite and not negative, ``clip`` inside (0, 1), ``clip_vf`` finite and positive, ``ent_coef`` finite and not negative;
    ``total`` an integer in 0 .. 2^53 - 1; ``kl_stop`` 0 (no stop) or finite and positive.  Needs no device."""
    if isinstance(total, bool) or not isinstance(total, (int, np.integer)) or not 0 <= int(total) < 2 ** 53:
        raise ValueError("total must be an integer in 0 .. 2^53 - 1, got %r" % (total,))
    lr, clip, clip_vf, ent_coef = (_sched_pair(w, x) for w, x in (("lr", lr), ("clip", clip), ("clip_vf", clip_vf), ("ent_coef", ent_coef)))
    for x in lr:
        if not np.isfinite(x) or x < 0.0:
            raise ValueError("lr must be finite and not negative")
    for x in clip:
        if not (np.isfinite(x) and 0.0 < x < 1.0):
            raise ValueError("clip must be inside (0, 1)")
    for x in clip_vf:
        if not np.isfinite(x) or not (x > 0.0):
            raise ValueError("clip_vf must be finite and positive")
    for x in ent_coef:
        if not np.isfinite(x) or x < 0.0:
            raise ValueError("ent_coef must be finite and not negative")
    if isinstance(kl_stop, bool):
        raise ValueError("kl_stop must be 0 or a positive number")
    kl_stop = float(kl_stop)
    if not np.isfinite(kl_stop) or kl_stop < 0.0:
        raise ValueError("kl_stop must be 0 (no stop) or finite and positive")
    return int(total), lr, clip, clip_vf, ent_coef, kl_stop


def pg_schedule_ref(it, total, a, b):
    """The rule of ``bsk_fit_schedule_begin`` restated -> numpy.float64: ``a`` exactly while ``total`` == 0 or ``it`` == 0, ``b``
    exactly - not a + (b - a) - from ``it`` >= ``total`` on, and between them a + (b - a) * (float64(it) / float64(total)), every
    operation rounded on its own.  ``it`` and ``total`` integers, ``total`` below 2^53.  Bit for bit the device's."""
    it, total = int(it), int(total)
    if it < 0 or not 0 <= total < 2 ** 53:
        raise ValueError("it must not be negative and total must be in 0 .. 2^53 - 1")
    a, b = np.float64(a), np.float64(b)
    if total == 0 or it == 0:
        return a
    if it >= total:
        return b
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        frac = np.float64(it) / np.float64(total)
        span = b - a
        return a + span * frac


def fit_kl_gate_ref(rows, kl_stop, gate=0, skipped=0, kl_at_stop=0.0):
    """``bsk_fit_kl_gate`` restated -> (gate, skipped, kl_at_stop, mean): the three words behind the launch and the minibatch's mean
    KL.  ``rows`` float64 (n_rows, 8) in the loop's ``log`` layout - ``PG_STATS_COLUMNS`` then ``FIT_STATS_COLUMNS``: S = column 0
    and N = column 7, each summed ascending FROM the first row; mean = S / N.  A closed gate stays closed; an open one closes when
    N > 0 and not (mean <= kl_stop) - a NaN closes it, a mean exactly at ``kl_stop`` does not - and that transition alone sets
    ``kl_at_stop`` = mean.  Closed, now or earlier: skipped + 1, and the caller's accumulation is dropped (the fit's count = 0)."""
    rows = np.asarray(rows, np.float64)
    if rows.ndim != 2 or rows.shape[1] != 8 or rows.shape[0] < 1:
        raise ValueError("rows: (n_rows, 8), n_rows >= 1")
    gate, skipped, kl_at_stop = int(gate), int(skipped), np.float64(kl_at_stop)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        S, N = rows[0, 0], rows[0, 7]
        for r in range(1, rows.shape[0]):
            S, N = S + rows[r, 0], N + rows[r, 7]
        mean = S / N
    if gate == 0 and N > 0.0 and not (mean <= np.float64(kl_stop)):
        gate, kl_at_stop = 1, mean
    if gate:
        skipped = (skipped + 1) % 2 ** 64
    return gate, skipped, kl_at_stop, mean


def sched_words_ref(it, total, lr, clip, clip_vf, ent_coef):
    """The eight words ``bsk_fit_schedule_begin`` leaves at iteration ``it`` -> uint64 (8,): the four values by ``pg_schedule_ref``
    as the bits of float64 numbers, the iteration, and the gate open (three zero words)."""
    words = np.zeros(SCHED_WORDS, np.uint64)
    words.view(np.float64)[:4] = [pg_schedule_ref(it, total, *pair) for pair in (lr, clip, clip_vf, ent_coef)]
    words[4] = int(it)
    return words


def sched_log_table_ref(rows):
    """The schedule's ring as the device holds it -> float64 (k, 8): the rows of ``SCHED_LOG_COLUMNS`` that have been written (the
    iteration is not a NaN), oldest first."""
    rows = np.asarray(rows, np.float64).reshape(-1, len(SCHED_LOG_COLUMNS))
    valid = np.flatnonzero(~np.isnan(rows[:, 0]))
    return rows[valid[np.argsort(rows[valid, 0], kind="stable")]].copy()
