"""A small MLP policy evaluated on the GPU by the library itself, and closed-loop rollouts built from it.

``DevicePolicy`` holds one or two multilayer perceptrons over the five observation rows (``bsk_policy_*``, include/bskgpu.h): the
action network (5 -> hidden... -> 3 logits) and an optional value network (5 -> hidden... -> 1).  ``act`` is ONE launch that reads
the observation rows where the step kernel leaves them and writes int32 actions ``step_device`` reads in place (plus, when asked,
log-probability, value and logits); ``rollout`` closes the loop on the device for whole episodes.  Both are enqueue-only and can be
captured into a HIP graph.  An extra beside the reference surface: the reference's agent runs its network in
stable-baselines, outside the env.

The arithmetic is fixed to the bit (include/bskgpu.h): every layer output is one k-ordered chain of f32 fused multiply-adds from
the bias.  ``mlp_ref`` / ``act_ref`` restate it in numpy - for ``relu`` networks logits, value and greedy actions come out equal
to the kernel's bit for bit - and need no device, like the argument rules.

``PolicyPopulation`` holds P parameter sets of one spec (``bsk_population_*``): member m drives envs [m * E, (m + 1) * E) of one
propagator, one launch per env step serves all members, and the per-member fitness of a rollout is formed on the device
(``population_fitness_ref`` restates it in numpy, bit for bit).  ``EvolutionStrategy`` is the host-side loop around it;
``DeviceEvolutionStrategy`` (``bsk_es_*``) keeps theta on the device and asks, ranks and updates there, its noise regenerated from
a counter instead of stored (``es_noise_ref`` / ``es_ask_ref`` / ``es_tell_ref`` restate it in numpy, bit for bit).
"""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import POLICY_GREEDY, POLICY_RELU, POLICY_SAMPLE, POLICY_TANH, BskPolicySpec, check

MAX_HIDDEN_LAYERS = 3
ACTIVATIONS = {"relu": POLICY_RELU, "tanh": POLICY_TANH}
MODES = {"greedy": POLICY_GREEDY, "sample": POLICY_SAMPLE}

#: hidden: widths of the action network's hidden layers; value_hidden: the value network's, or None (no value network)
Spec = namedtuple("Spec", "hidden activation value_hidden value_activation")


def _check_net(hidden, activation, what):
    hidden = tuple(hidden)
    if len(hidden) > MAX_HIDDEN_LAYERS:
        raise ValueError("%s: 0 to %d hidden layers, got %d" % (what, MAX_HIDDEN_LAYERS, len(hidden)))
    for w in hidden:
        if not (isinstance(w, (int, np.integer)) and 16 <= w <= 128 and w % 16 == 0):
            raise ValueError("%s: a hidden layer is 16 ... 128 units wide in multiples of 16, got %r" % (what, w))
    if activation not in ACTIVATIONS:
        raise ValueError("%s: activation must be 'relu' or 'tanh', got %r" % (what, activation))
    return tuple(int(w) for w in hidden)


def check_spec(hidden, activation="relu", value_hidden=None, value_activation=None):
    """Argument rules of a policy (no device needed) -> ``Spec``.  ``value_hidden=None``: no value network; its activation
    defaults to the action network's."""
    hidden = _check_net(hidden, activation, "action network")
    if value_hidden is None:
        if value_activation is not None:
            raise ValueError("value_activation given without a value network")
        return Spec(hidden, activation, None, None)
    value_activation = activation if value_activation is None else value_activation
    return Spec(hidden, activation, _check_net(value_hidden, value_activation, "value network"), value_activation)


def _as_spec(spec):
    return spec if isinstance(spec, Spec) else check_spec(*spec)


def c_spec(spec):
    """``Spec`` -> the C-ABI's ``bsk_policy_spec``."""
    spec = _as_spec(spec)
    c = BskPolicySpec()
    c.abi_version, c.struct_size = _lib.BSK_ABI_VERSION, C.sizeof(BskPolicySpec)
    c.n_hidden, c.activation = len(spec.hidden), ACTIVATIONS[spec.activation]
    for k, w in enumerate(spec.hidden):
        c.hidden[k] = w
    if spec.value_hidden is not None:
        c.has_value, c.v_n_hidden, c.v_activation = 1, len(spec.value_hidden), ACTIVATIONS[spec.value_activation]
        for k, w in enumerate(spec.value_hidden):
            c.v_hidden[k] = w
    return c


def layer_shapes(spec):
    """-> ([(out, in), ...] of the action network, the same of the value network or None)."""
    spec = _as_spec(spec)

    def net(hidden, n_out):
        widths = (5,) + tuple(hidden) + (n_out,)
        return [(widths[k + 1], widths[k]) for k in range(len(widths) - 1)]
    return net(spec.hidden, 3), (None if spec.value_hidden is None else net(spec.value_hidden, 1))


def n_params(spec):
    """Floats in the parameter block: in_scale[5], in_shift[5], then W[out][in] and b[out] per layer (``bsk_policy_n_params``)."""
    a, v = layer_shapes(spec)
    return 10 + sum(o * i + o for o, i in a + (v or []))


def pack_params(spec, layers, value_layers=None, in_scale=None, in_shift=None):
    """The parameter block of include/bskgpu.h as one float32 array: ``in_scale[5]``, ``in_shift[5]`` (default 1 and 0), then per
    layer ``W[out][in]`` row-major (``nn.Linear.weight``) and ``b[out]``; the action network's ``layers`` = [(W, b), ...] first,
    then ``value_layers``."""
    spec = _as_spec(spec)
    a, v = layer_shapes(spec)
    if (v is None) != (value_layers is None):
        raise ValueError("value_layers must be given exactly when the spec has a value network")
    parts = [np.ones(5, np.float32) if in_scale is None else np.asarray(in_scale, np.float32).reshape(-1),
             np.zeros(5, np.float32) if in_shift is None else np.asarray(in_shift, np.float32).reshape(-1)]
    if parts[0].shape != (5,) or parts[1].shape != (5,):
        raise ValueError("in_scale and in_shift have 5 entries each")
    for shapes, given, what in ((a, layers, "layers"), (v, value_layers, "value_layers")):
        if shapes is None:
            continue
        given = list(given)
        if len(given) != len(shapes):
            raise ValueError("%s: expected %d (W, b) pairs, got %d" % (what, len(shapes), len(given)))
        for (o, i), (W, b) in zip(shapes, given):
            W, b = np.asarray(W, np.float32), np.asarray(b, np.float32)
            if W.shape != (o, i) or b.shape != (o,):
                raise ValueError("%s: expected W %r and b %r, got %r and %r" % (what, (o, i), (o,), W.shape, b.shape))
            parts += [W.reshape(-1), b]
    return np.ascontiguousarray(np.concatenate(parts))


def unpack_params(spec, params):
    """-> in_scale (5,), in_shift (5,), [(W, b), ...] of the action network, the same of the value network or None."""
    spec = _as_spec(spec)
    p = np.asarray(params, np.float32).reshape(-1)
    if p.size != n_params(spec):
        raise ValueError("expected %d parameters, got %d" % (n_params(spec), p.size))
    at = [10]

    def net(shapes):
        out = []
        for o, i in shapes:
            W = p[at[0]:at[0] + o * i].reshape(o, i)
            b = p[at[0] + o * i:at[0] + o * i + o]
            at[0] += o * i + o
            out.append((W, b))
        return out
    a, v = layer_shapes(spec)
    return p[:5], p[5:10], net(a), (None if v is None else net(v))


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


def torch_layers(module):
    """An ``nn.Sequential`` of ``Linear`` / ``ReLU`` / ``Tanh`` -> (hidden widths, activation, [(W, b), ...] as float32 numpy).
    Every ``Linear`` but the last is followed by one activation, the same one throughout; anything else is a ``ValueError``."""
    import torch.nn as nn
    mods = list(module) if isinstance(module, nn.Sequential) else None
    if not mods:
        raise ValueError("expected a non-empty nn.Sequential of Linear / ReLU / Tanh")
    layers, acts, expect_linear = [], set(), True
    for m in mods:
        if expect_linear and isinstance(m, nn.Linear):
            W = m.weight.detach().cpu().float().numpy()
            b = m.bias.detach().cpu().float().numpy() if m.bias is not None else np.zeros(W.shape[0], np.float32)
            layers.append((np.ascontiguousarray(W), np.ascontiguousarray(b)))
            expect_linear = False
        elif not expect_linear and type(m) in (nn.ReLU, nn.Tanh):
            acts.add("relu" if type(m) is nn.ReLU else "tanh")
            expect_linear = True
        else:
            raise ValueError("unsupported module sequence at %r: Linear layers, each but the last followed by ReLU or Tanh" % (m,))
    if expect_linear:
        raise ValueError("the network must end with a Linear layer")
    if len(acts) > 1:
        raise ValueError("one hidden activation per network: found both ReLU and Tanh")
    return tuple(W.shape[0] for W, _ in layers[:-1]), (acts.pop() if acts else "relu"), layers


class _ViewOwner(object):
    """What a view of the policy's output buffers keeps alive - the policy, which owns them - and waits for when a consumer on
    another stream takes the view (the propagator's stream, where the launch went)."""

    def __init__(self, policy, prop):
        self.policy, self.prop = policy, prop

    def sync(self):
        self.prop.sync()


def _observation_source(pol, source, env_base, stream):
    """What ``act`` evaluates: a ``BatchedPropagator`` (or an env with a ``propagator``) - its own observation buffers, stream and
    env_base - or a device array (5, n) float64 with contiguous rows.  -> (pointer, row stride, n, stream, env_base, owner of the
    output views); ``pol`` is the policy or population that acts."""
    prop = getattr(source, "propagator", source)
    if hasattr(prop, "device_views") and hasattr(prop, "stream_ptr"):
        if prop.device != pol.device:
            raise ValueError("the policy lives on device %d, the propagator on device %d" % (pol.device, prop.device))
        v = prop.device_views()
        ptr, stride, n = v["obs"].__cuda_array_interface__["data"][0], v["stride"], prop.n_envs
        stream = prop.stream_ptr() if stream is None else stream
        env_base = getattr(prop, "env_base", 0) if env_base is None else env_base
        owner = _ViewOwner(pol, prop)
    else:
        cai = getattr(source, "__cuda_array_interface__", None)
        if cai is None:
            raise TypeError("expected a BatchedPropagator or a device array with __cuda_array_interface__, got %r" % type(source))
        shape, strides = tuple(cai["shape"]), cai.get("strides")
        if cai["typestr"] != "<f8" or len(shape) != 2 or shape[0] != 5 or shape[1] < 1:
            raise ValueError("observations: a float64 device array of shape (5, n), got %r %r" % (cai["typestr"], shape))
        strides = (shape[1] * 8, 8) if strides is None else tuple(strides)
        if strides[1] != 8 or strides[0] % 8 or strides[0] < shape[1] * 8:
            raise ValueError("observations: rows must be contiguous and at least n elements apart")
        ptr, stride, n = int(cai["data"][0]), strides[0] // 8, shape[1]
        owner = pol
        pol._source = source                   # (the launch reads it after this call returns)
    return ptr, stride, n, int(stream or 0), int(env_base or 0), owner


class DevicePolicy(object):
    """The policy on one GPU.  ``spec``: a ``Spec`` (``check_spec``); ``params``: its float32 parameter block (``pack_params``).
    Not thread-safe, and one stream at a time: the draw counter and the output buffers are single.  Output buffers are sized for
    the largest batch seen so far; a call that must grow them allocates, so make the first call of a size outside a graph capture."""

    def __init__(self, spec, params, device=0):
        self.spec = _as_spec(spec)
        p = np.ascontiguousarray(params, dtype=np.float32).reshape(-1)
        if p.size != n_params(self.spec):
            raise ValueError("expected %d parameters, got %d" % (n_params(self.spec), p.size))
        self._lib = _lib.load()
        self.device = int(device)
        self._cs = c_spec(self.spec)
        h = C.c_void_p()
        check(self._lib.bsk_policy_create(C.byref(self._cs), p.ctypes.data, self.device, C.byref(h)))
        self._p = h
        self._out, self._out_n, self._source = None, 0, None

    @classmethod
    def from_torch(cls, module, value_module=None, in_scale=None, in_shift=None, device=0):
        """From an ``nn.Sequential`` of ``Linear`` / ``ReLU`` / ``Tanh`` (5 inputs, 3 outputs) and, optionally, one for the value
        (5 inputs, 1 output).  Weights are cast to float32."""
        hidden, act, layers = torch_layers(module)
        vh = va = vl = None
        if value_module is not None:
            vh, va, vl = torch_layers(value_module)
        spec = check_spec(hidden, act, vh, va)
        return cls(spec, pack_params(spec, layers, vl, in_scale, in_shift), device=device)

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_p", None):
            self._lib.bsk_policy_destroy(self._p)
            self._p = None
        for b in (getattr(self, "_out", None) or {}).values():
            b.free()
        self._out = self._source = None

    def __del__(self):
        try:
            import sys
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._p:
            raise RuntimeError("policy is closed")
        return self._p

    def sync(self):
        """Waits for everything queued on the policy's device (the policy keeps no stream of its own)."""
        from . import _hip
        with _hip.device_guard(self.device):
            _hip.check(_hip.runtime().hipDeviceSynchronize(), "hipDeviceSynchronize")

    def set_params(self, params):
        p = np.ascontiguousarray(params, dtype=np.float32).reshape(-1)
        if p.size != n_params(self.spec):
            raise ValueError("expected %d parameters, got %d" % (n_params(self.spec), p.size))
        check(self._lib.bsk_policy_set_params(self._handle(), p.ctypes.data))

    def set_rng(self, seed, draw=0):
        check(self._lib.bsk_policy_set_rng(self._handle(), int(seed), int(draw)))

    def get_rng(self):
        """-> (seed, draw); synchronises."""
        s, d = C.c_uint64(), C.c_uint64()
        check(self._lib.bsk_policy_get_rng(self._handle(), C.byref(s), C.byref(d)))
        return s.value, d.value

    # ------------------------------------------------------------------ evaluation
    def _buffers(self, n):
        if self._out is None or self._out_n < n:
            from . import _hip
            if self._out:
                self.sync()
                for b in self._out.values():
                    b.free()
            self._out = {"action": _hip.DeviceBuffer(4 * n, self.device), "logp": _hip.DeviceBuffer(4 * n, self.device),
                         "value": _hip.DeviceBuffer(4 * n, self.device), "logits": _hip.DeviceBuffer(12 * n, self.device)}
            self._out_n = n
        return self._out

    def enqueue(self, obs_ptr, obs_stride, n, mode="greedy", want=(), env_base=0, stream=0):
        """``bsk_policy_act`` on raw arguments (what ``act`` resolves its source to, for loops that resolve it once): observations
        f64[5][obs_stride] at ``obs_ptr``.  -> the policy's output buffers by name (``_hip.DeviceBuffer``: ``action`` int32[n],
        ``logp`` / ``value`` f32[n], ``logits`` f32[3][n]); only ``action`` and the names in ``want`` are written."""
        if mode not in MODES:
            raise ValueError("mode must be 'greedy' or 'sample'")
        out = self._buffers(int(n))
        vp = lambda name: C.c_void_p(out[name].ptr) if name in want else None      # noqa: E731
        check(self._lib.bsk_policy_act(self._handle(), C.c_void_p(int(obs_ptr)), int(obs_stride), int(n), int(env_base), MODES[mode],
                                       C.c_void_p(out["action"].ptr), vp("logp"), vp("value"), vp("logits"), int(n), C.c_void_p(int(stream))))
        return out

    def act(self, source, mode="greedy", want=("logp", "value", "logits"), env_base=None, stream=None):
        """One launch: actions (and what ``want`` names) for every spacecraft of ``source`` - a ``BatchedPropagator`` (or an env
        with a ``propagator``): its own observation buffers, stream and env_base - or any device array of shape (5, n) float64 with
        contiguous rows (``__cuda_array_interface__``: a torch tensor, a propagator view), evaluated on ``stream`` (an integer
        hipStream_t, default the null stream).  Enqueue-only: no copy, no synchronisation.
        -> dict of device views (``__cuda_array_interface__`` / DLPack) valid until the next call: ``action`` int32 (n,) - whose
        pointer ``step_device`` takes as it is - and ``logp`` (n,), ``value`` (n,), ``logits`` (3, n) float32 where wanted."""
        from .simulators.dynamics.propagator import _DevArray
        if mode not in MODES:
            raise ValueError("mode must be 'greedy' or 'sample'")
        want = tuple(want)
        for w in want:
            if w not in ("logp", "value", "logits"):
                raise ValueError("want: 'logp', 'value' and / or 'logits', got %r" % (w,))
        if "value" in want and self.spec.value_hidden is None:
            raise ValueError("want 'value': the policy has no value network")
        ptr, stride, n, stream, env_base, owner = _observation_source(self, source, env_base, stream)
        out = self.enqueue(ptr, stride, n, mode, want, env_base, stream)
        kw = {"owner": owner, "device": self.device, "stream": stream}
        res = {"action": _DevArray(out["action"].ptr, (n,), "<i4", **kw)}
        for name in want:
            res[name] = _DevArray(out[name].ptr, (3, n) if name == "logits" else (n,), "<f4", **kw)
        return res

    def rollout_device(self, prop, n_steps, substeps, mode="greedy", d_obs_hist=None, d_reward_hist=None, d_reason_hist=None,
                       d_action_hist=None, d_logp_hist=None, d_value_hist=None):
        """``bsk_policy_rollout`` with device pointers (or None) for the history rows: ``n_steps`` rounds of policy -> step -> history
        row enqueued on the propagator's stream, no copy, no synchronisation (capturable once a first rollout without
        ``d_action_hist`` has allocated the policy's scratch row)."""
        if mode not in MODES:
            raise ValueError("mode must be 'greedy' or 'sample'")
        prop = getattr(prop, "propagator", prop)
        vp = lambda p: C.c_void_p(int(p)) if p else None      # noqa: E731
        check(self._lib.bsk_policy_rollout(self._handle(), prop._handle(), MODES[mode], int(substeps), int(n_steps), vp(d_obs_hist),
                                           vp(d_reward_hist), vp(d_reason_hist), vp(d_action_hist), vp(d_logp_hist), vp(d_value_hist)))

    def rollout(self, prop, n_steps, substeps, mode="greedy"):
        """Closed-loop rollout with host results: -> dict of numpy arrays ``obs`` (n_steps, 5, n), ``reward`` (n_steps, n), ``reason``
        (n_steps, n) uint8 - ``step_n``'s rows - and ``action`` int32, ``logp`` float32, ``value`` float32 (with a value network)
        (n_steps, n) of the observation each action was chosen FROM.  Allocates device scratch per call and synchronises: the
        convenience form; a training process hands ``rollout_device`` its own buffers."""
        from . import _hip
        prop = getattr(prop, "propagator", prop)
        n, T = prop.n_envs, int(n_steps)
        names = [("obs", np.float64, (T, 5, n)), ("reward", np.float64, (T, n)), ("reason", np.uint8, (T, n)),
                 ("action", np.int32, (T, n)), ("logp", np.float32, (T, n))]
        if self.spec.value_hidden is not None:
            names.append(("value", np.float32, (T, n)))
        host = {k: np.empty(shape, dtype=dt) for k, dt, shape in names}
        bufs = {k: _hip.DeviceBuffer(host[k].nbytes, self.device) for k in host}
        try:
            self.rollout_device(prop, T, substeps, mode, bufs["obs"].ptr, bufs["reward"].ptr, bufs["reason"].ptr, bufs["action"].ptr,
                                bufs["logp"].ptr, bufs["value"].ptr if "value" in bufs else None)
            stream = C.c_void_p(prop.stream_ptr())
            for k, dst in host.items():
                _hip.check(_hip.runtime().hipMemcpyAsync(C.c_void_p(dst.ctypes.data), C.c_void_p(bufs[k].ptr), dst.nbytes,
                                                         _hip.hipMemcpyDeviceToHost, stream), "hipMemcpyAsync")
            prop.sync()
        finally:
            for b in bufs.values():
                b.free()
        return host


# ---------------------------------------------------------------------------------------------------------------------------------
# Populations: P parameter sets on the device, member m driving envs [m * E, (m + 1) * E) of one handle (bsk_population_*)

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


class PolicyPopulation(object):
    """``n_members`` parameter sets of one ``spec`` on one GPU.  With ``envs_per_member`` = E (a multiple of 64), spacecraft j is
    driven by member j // E: ONE policy launch per env step serves every member, and ``rollout_device`` / ``evaluate`` form the
    per-member fitness on the device.  ``params``: float32 (P, n_params), one ``pack_params`` block per row, or None with
    ``n_members`` given (all-zero members).  Not thread-safe, one stream at a time, like ``DevicePolicy``."""

    def __init__(self, spec, params=None, device=0, n_members=None):
        self.spec = _as_spec(spec)
        self.n_params = n_params(self.spec)
        if params is None:
            if n_members is None:
                raise ValueError("give params (P, n_params) or n_members")
            p, self.n_members = None, int(n_members)
        else:
            p = self._blocks(params, None)
            self.n_members = p.shape[0]
            if n_members is not None and int(n_members) != self.n_members:
                raise ValueError("params has %d rows, n_members is %d" % (self.n_members, n_members))
        self._lib = _lib.load()
        self.device = int(device)
        self._cs = c_spec(self.spec)
        h = C.c_void_p()
        check(self._lib.bsk_population_create(C.byref(self._cs), self.n_members, None if p is None else p.ctypes.data, self.device,
                                              C.byref(h)))
        self._p = h
        self._out, self._out_n, self._source = None, 0, None

    def _blocks(self, params, count):
        p = np.ascontiguousarray(params, dtype=np.float32)
        if p.ndim != 2 or p.shape[1] != self.n_params or p.shape[0] < 1 or (count is not None and p.shape[0] != count):
            raise ValueError("expected parameters of shape (%s, %d), got %r" % ("P" if count is None else count, self.n_params, p.shape))
        return p

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_p", None):
            self._lib.bsk_population_destroy(self._p)
            self._p = None
        for b in (getattr(self, "_out", None) or {}).values():
            b.free()
        self._out = self._source = None

    def __del__(self):
        try:
            import sys
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._p:
            raise RuntimeError("population is closed")
        return self._p

    def sync(self):
        """Waits for everything queued on the population's device (it keeps no stream of its own)."""
        from . import _hip
        with _hip.device_guard(self.device):
            _hip.check(_hip.runtime().hipDeviceSynchronize(), "hipDeviceSynchronize")

    # ------------------------------------------------------------------ parameters
    def set_params(self, params):
        """All members from a host array (P, n_params); synchronises the device."""
        p = self._blocks(params, self.n_members)
        check(self._lib.bsk_population_set_params(self._handle(), p.ctypes.data))

    def set_params_device(self, src, first=0, count=None, stream=0):
        """Members ``first .. first + count - 1`` from DEVICE memory: ``src`` a raw pointer to ``count`` blocks of n_params float32
        (``count`` defaults to the members from ``first`` on), or anything with ``__cuda_array_interface__`` - a contiguous float32
        array of (count, n_params) or count * n_params elements.  One launch on ``stream``: no copy, no synchronisation,
        capturable.  A source array must stay alive until the launch has run."""
        cai = getattr(src, "__cuda_array_interface__", None)
        if cai is not None:
            size = int(np.prod(cai["shape"])) if len(cai["shape"]) else 1
            if cai["typestr"] != "<f4" or size % self.n_params or size == 0:
                raise ValueError("device parameters: float32, a multiple of %d elements, got %r %r" % (self.n_params, cai["typestr"], cai["shape"]))
            shape, strides = tuple(cai["shape"]), cai.get("strides")
            dense = tuple(4 * int(np.prod(shape[k + 1:], dtype=np.int64)) for k in range(len(shape)))
            if strides is not None and tuple(strides) != dense:
                raise ValueError("device parameters must be contiguous")
            if count is None:
                count = size // self.n_params
            elif int(count) * self.n_params != size:
                raise ValueError("device parameters: %d members need %d elements, got %d" % (count, int(count) * self.n_params, size))
            self._source = src
            src = cai["data"][0]
        if count is None:
            count = self.n_members - int(first)
        check(self._lib.bsk_population_set_params_device(self._handle(), C.c_void_p(int(src)) if src else None, int(first), int(count),
                                                         C.c_void_p(int(stream or 0))))

    def member(self, m):
        """Member ``m``'s parameter block (n_params,) float32 - what ``DevicePolicy(spec, block)`` takes.  Synchronises."""
        out = np.empty(self.n_params, np.float32)
        check(self._lib.bsk_population_get_member(self._handle(), int(m), out.ctypes.data))
        return out

    def set_rng(self, seed, draw=0):
        check(self._lib.bsk_population_set_rng(self._handle(), int(seed), int(draw)))

    def get_rng(self):
        """-> (seed, draw); synchronises."""
        s, d = C.c_uint64(), C.c_uint64()
        check(self._lib.bsk_population_get_rng(self._handle(), C.byref(s), C.byref(d)))
        return s.value, d.value

    # ------------------------------------------------------------------ evaluation
    _buffers = DevicePolicy._buffers

    def act(self, source, envs_per_member=None, mode="greedy", want=("logp", "value", "logits"), env_base=None, stream=None):
        """``DevicePolicy.act`` under the member rule: spacecraft j of ``source`` (a propagator, or a device array (5, n) float64)
        is evaluated with member j // envs_per_member (default n // n_members).  One launch, enqueue-only.  -> the same dict of
        device views."""
        from .simulators.dynamics.propagator import _DevArray
        if mode not in MODES:
            raise ValueError("mode must be 'greedy' or 'sample'")
        want = tuple(want)
        for w in want:
            if w not in ("logp", "value", "logits"):
                raise ValueError("want: 'logp', 'value' and / or 'logits', got %r" % (w,))
        if "value" in want and self.spec.value_hidden is None:
            raise ValueError("want 'value': the population has no value network")
        ptr, stride, n, stream, env_base, owner = _observation_source(self, source, env_base, stream)
        E = n // self.n_members if envs_per_member is None else int(envs_per_member)
        out = self._buffers(n)
        vp = lambda name: C.c_void_p(out[name].ptr) if name in want else None      # noqa: E731
        check(self._lib.bsk_population_act(self._handle(), C.c_void_p(ptr), stride, n, E, env_base, MODES[mode],
                                           C.c_void_p(out["action"].ptr), vp("logp"), vp("value"), vp("logits"), n, C.c_void_p(stream)))
        kw = {"owner": owner, "device": self.device, "stream": stream}
        res = {"action": _DevArray(out["action"].ptr, (n,), "<i4", **kw)}
        for name in want:
            res[name] = _DevArray(out[name].ptr, (3, n) if name == "logits" else (n,), "<f4", **kw)
        return res

    def rollout_device(self, prop, n_steps, substeps, mode="greedy", gamma=1.0, d_obs_hist=None, d_reward_hist=None, d_reason_hist=None,
                       d_action_hist=None, d_logp_hist=None, d_value_hist=None, d_env_value=None, d_env_len=None, d_fitness=None,
                       d_mean_len=None):
        """``bsk_population_rollout`` with device pointers (or None): one generation on the propagator's stream - per env step the
        policy launch for every member, the step, and one launch for the history rows and the running values; then the fitness
        (``d_env_value`` f64[n], ``d_env_len`` i32[n], ``d_fitness`` f64[P], ``d_mean_len`` f64[P]).  No copy, no synchronisation;
        capturable after a first rollout of the size has allocated the population's scratch rows."""
        if mode not in MODES:
            raise ValueError("mode must be 'greedy' or 'sample'")
        prop = getattr(prop, "propagator", prop)
        vp = lambda p: C.c_void_p(int(p)) if p else None      # noqa: E731
        check(self._lib.bsk_population_rollout(self._handle(), prop._handle(), MODES[mode], int(substeps), int(n_steps), float(gamma),
                                               vp(d_obs_hist), vp(d_reward_hist), vp(d_reason_hist), vp(d_action_hist), vp(d_logp_hist),
                                               vp(d_value_hist), vp(d_env_value), vp(d_env_len), vp(d_fitness), vp(d_mean_len)))

    def evaluate(self, prop, n_steps, substeps, mode="greedy", gamma=1.0):
        """One generation with host results: -> dict ``fitness`` (P,), ``mean_len`` (P,), ``env_value`` (n,) float64 and ``env_len``
        (n,) int32.  Allocates device scratch per call and synchronises: the convenience form; a search loop that keeps its
        candidates on the device hands ``rollout_device`` its own buffers."""
        from . import _hip
        prop = getattr(prop, "propagator", prop)
        n, P = prop.n_envs, self.n_members
        host = {"env_value": np.empty(n, np.float64), "env_len": np.empty(n, np.int32), "fitness": np.empty(P, np.float64),
                "mean_len": np.empty(P, np.float64)}
        bufs = {k: _hip.DeviceBuffer(a.nbytes, self.device) for k, a in host.items()}
        try:
            self.rollout_device(prop, n_steps, substeps, mode, gamma, d_env_value=bufs["env_value"].ptr, d_env_len=bufs["env_len"].ptr,
                                d_fitness=bufs["fitness"].ptr, d_mean_len=bufs["mean_len"].ptr)
            stream = C.c_void_p(prop.stream_ptr())
            for k, dst in host.items():
                _hip.check(_hip.runtime().hipMemcpyAsync(C.c_void_p(dst.ctypes.data), C.c_void_p(bufs[k].ptr), dst.nbytes,
                                                         _hip.hipMemcpyDeviceToHost, stream), "hipMemcpyAsync")
            prop.sync()
        finally:
            for b in bufs.values():
                b.free()
        return host


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
# The evolution strategy on the device (bsk_es_*; definition in include/bskgpu.h, kernels in csrc/bsk_es.hip) and its restatement

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


def _es_pair_sum(fitness, n_params, seed, generation):
    """Steps 1 - 3 of ``bsk_es_tell`` up to s[0] -> (float64 (n_params,), P): the one sum behind ``es_tell_ref`` and
    ``es_tell_adam_ref``, as ``ES_PAIR_SUM`` (csrc/bsk_es.hip) is behind the two update kernels."""
    u = centred_ranks(fitness)
    P = u.size
    if P < 2 or P % 2:
        raise ValueError("expected an even number of fitness values, at least 2")
    w = u[0::2] - u[1::2]
    with np.errstate(invalid="ignore", over="ignore"):
        terms = w[:, None] * es_noise_ref(seed, generation, P // 2, n_params)
        s = np.zeros((64, int(n_params)), np.float64)
        s[:min(64, P // 2)] = terms[:64]
        for at in range(64, P // 2, 64):
            chunk = terms[at:at + 64]
            s[:len(chunk)] = s[:len(chunk)] + chunk
        for stride in (32, 16, 8, 4, 2, 1):
            s[:stride] = s[:stride] + s[stride:2 * stride]
    return s[0].copy(), P


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
    a1, a2 = np.float64(1.0) - b1, np.float64(1.0) - b2
    p1, p2 = bp[0] * b1, bp[1] * b2
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = theta[frozen:]
        g = cg * s0[frozen:] - wd * t
        mj = b1 * m[frozen:] + a1 * g
        vj = b2 * v[frozen:] + (a2 * g) * g
        m[frozen:], v[frozen:] = mj, vj
        theta[frozen:] = t + (lr * (mj / (np.float64(1.0) - p1))) / (np.sqrt(vj / (np.float64(1.0) - p2)) + eps)
    return theta, m, v, np.array([p1, p2], np.float64)


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


class DeviceEvolutionStrategy(object):
    """``EvolutionStrategy``'s search with theta, the ranking and the update on the device (``bsk_es_*``): ``ask`` writes the
    ``population`` = P members straight into a ``PolicyPopulation``'s device layout, ``tell`` reads the P float64 fitness values
    a rollout left in device memory; both are enqueue-only and capturable, and the noise is regenerated from (seed, generation,
    pair, parameter) instead of stored.  ``theta``: the float32 parameter block the search starts from (None: zeros).  Equal bit
    for bit to ``es_ask_ref`` / ``es_tell_ref``.  ``optimizer="adam"`` drives the same estimate through Adam with the L2 penalty
    ``weight_decay`` (``bsk_es_set_optimizer``; ``es_tell_adam_ref``); ``"sgd"``, the default, ignores the four Adam arguments.
    Not thread-safe, one stream at a time."""

    def __init__(self, spec, theta, population, sigma=0.1, lr=0.05, seed=0, frozen=10, device=0, optimizer="sgd", beta1=0.9,
                 beta2=0.999, eps=1e-8, weight_decay=0.0):
        if optimizer not in ("sgd", "adam"):
            raise ValueError("optimizer must be 'sgd' or 'adam', got %r" % (optimizer,))
        if optimizer == "adam":
            beta1, beta2, eps, weight_decay = check_adam(beta1, beta2, eps, weight_decay)
        self.optimizer, self.adam = optimizer, (beta1, beta2, eps, weight_decay)
        self.spec = _as_spec(spec)
        self.n_params = n_params(self.spec)
        self.population, self.sigma, self.lr, self.frozen = int(population), float(sigma), float(lr), int(frozen)
        self.seed, self.device = int(seed), int(device)
        t = None
        if theta is not None:
            t = np.ascontiguousarray(theta, dtype=np.float32).reshape(-1)
            if t.size != self.n_params:
                raise ValueError("expected %d parameters, got %d" % (self.n_params, t.size))
        self._lib = _lib.load()
        self._cs = c_spec(self.spec)
        h = C.c_void_p()
        check(self._lib.bsk_es_create(C.byref(self._cs), self.population, None if t is None else t.ctypes.data, self.sigma, self.lr,
                                      self.frozen, self.seed, self.device, C.byref(h)))
        self._p = h
        self._fitness = self._source = None
        if optimizer == "adam":
            self.set_optimizer("adam", beta1, beta2, eps, weight_decay)

    # ------------------------------------------------------------------ lifecycle
    def close(self):
        if getattr(self, "_p", None):
            self._lib.bsk_es_destroy(self._p)
            self._p = None
        if getattr(self, "_fitness", None) is not None:
            self._fitness.free()
        self._fitness = self._source = None

    def __del__(self):
        try:
            import sys
            if sys.is_finalizing():
                return
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._p:
            raise RuntimeError("evolution strategy is closed")
        return self._p

    # ------------------------------------------------------------------ state
    @property
    def theta(self):
        """float64 (n_params,); synchronises."""
        out = np.empty(self.n_params, np.float64)
        check(self._lib.bsk_es_get_state(self._handle(), out.ctypes.data, None))
        return out

    @property
    def generation(self):
        """The generation the next ``ask`` / ``tell`` draw their noise for; synchronises."""
        g = C.c_uint64()
        check(self._lib.bsk_es_get_state(self._handle(), None, C.byref(g)))
        return g.value

    def set_state(self, theta=None, generation=0):
        """New theta (float64 (n_params,), or None: keep) and generation counter; synchronises."""
        t = None
        if theta is not None:
            t = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1)
            if t.size != self.n_params:
                raise ValueError("expected %d parameters, got %d" % (self.n_params, t.size))
        check(self._lib.bsk_es_set_state(self._handle(), None if t is None else t.ctypes.data, int(generation)))

    def generation_ptr(self):
        """The generation counter as a DEVICE uint64 word, valid until ``close``: the epoch of ``reset_from_pool_shared``."""
        p = C.c_void_p()
        check(self._lib.bsk_es_generation_device(self._handle(), C.byref(p)))
        return p.value

    def set_optimizer(self, optimizer, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
        """``"adam"``: Adam with an L2 penalty from zero moments (every selection zeroes them); ``"sgd"``: the plain step.  Theta and
        the generation stay; synchronises."""
        if optimizer not in ("sgd", "adam"):
            raise ValueError("optimizer must be 'sgd' or 'adam', got %r" % (optimizer,))
        if optimizer == "adam":
            beta1, beta2, eps, weight_decay = check_adam(beta1, beta2, eps, weight_decay)
        check(self._lib.bsk_es_set_optimizer(self._handle(), _lib.ES_ADAM if optimizer == "adam" else _lib.ES_SGD, float(beta1), float(beta2),
                                             float(eps), float(weight_decay)))
        self.optimizer, self.adam = optimizer, (float(beta1), float(beta2), float(eps), float(weight_decay))

    @property
    def moments(self):
        """Adam's (m, v, beta_pow): float64 (n_params,), (n_params,), (2,); synchronises.  An error while the optimiser is SGD."""
        m, v, bp = np.empty(self.n_params, np.float64), np.empty(self.n_params, np.float64), np.empty(2, np.float64)
        check(self._lib.bsk_es_get_moments(self._handle(), m.ctypes.data, v.ctypes.data, bp.ctypes.data))
        return m, v, bp

    def set_moments(self, m=None, v=None, beta_pow=None):
        """New Adam moments (float64 (n_params,) each) and running powers (float64 (2,)); None keeps; synchronises."""
        arrs = []
        for a, size in ((m, self.n_params), (v, self.n_params), (beta_pow, 2)):
            if a is not None:
                a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
                if a.size != size:
                    raise ValueError("expected %d values, got %d" % (size, a.size))
            arrs.append(a)
        check(self._lib.bsk_es_set_moments(self._handle(), *[None if a is None else a.ctypes.data for a in arrs]))

    # ------------------------------------------------------------------ the search
    def ask(self, pop, stream=0):
        """This generation's members into every member of ``pop`` (a ``PolicyPopulation`` of the same spec and size): one launch
        on ``stream``, no copy, no synchronisation."""
        check(self._lib.bsk_es_ask(self._handle(), pop._handle(), C.c_void_p(int(stream or 0))))

    def tell(self, d_fitness, stream=0):
        """``d_fitness``: P float64 in DEVICE memory (greater is better) - a raw pointer or anything with
        ``__cuda_array_interface__``.  Ranks them, moves theta and advances the generation: three launches on ``stream``."""
        cai = getattr(d_fitness, "__cuda_array_interface__", None)
        if cai is not None:
            size = int(np.prod(cai["shape"])) if len(cai["shape"]) else 1
            strides = cai.get("strides")
            if cai["typestr"] != "<f8" or size != self.population or (strides is not None and len(cai["shape"]) == 1 and strides[0] != 8):
                raise ValueError("device fitness: %d contiguous float64, got %r %r" % (self.population, cai["typestr"], cai["shape"]))
            self._source = d_fitness
            d_fitness = cai["data"][0]
        check(self._lib.bsk_es_tell(self._handle(), C.c_void_p(int(d_fitness)) if d_fitness else None, C.c_void_p(int(stream or 0))))

    def fitness_buffer(self):
        """The device buffer of P float64 ``run_generation`` has the rollout write the fitness to (``_hip.DeviceBuffer``)."""
        if self._fitness is None:
            from . import _hip
            self._fitness = _hip.DeviceBuffer(8 * self.population, self.device)
        return self._fitness

    def run_generation(self, prop, pop, n_steps, substeps, mode="greedy", gamma=1.0, reset=True, shared_episodes=False):
        """One generation on the propagator's stream: every env restarted from the propagator's IC pool (``reset``; needs an
        auto-reset pool), ``ask``, ``pop.rollout_device`` with the fitness into ``fitness_buffer()``, ``tell``.  Nothing else is
        issued - no copy, no synchronisation - so after one warming call (it allocates the buffer and the population's scratch
        rows) a call can be captured into a graph and replayed generation after generation.  ``shared_episodes``: the reset is
        ``reset_from_pool_shared`` with E = n_envs // population and the generation word as the epoch, so that all members of a
        generation are scored on the same E initial conditions and every generation draws new ones; nothing else in the stream
        changes.  That is exact for ``greedy``: sample mode still draws its uniform per global env index."""
        prop = getattr(prop, "propagator", prop)
        fit = self.fitness_buffer()
        stream = prop.stream_ptr()
        if reset and shared_episodes:
            prop.reset_from_pool_shared(prop.n_envs // self.population, self.generation_ptr())
        elif reset:
            prop.reset_from_pool_device(None)
        self.ask(pop, stream)
        pop.rollout_device(prop, n_steps, substeps, mode, gamma, d_fitness=fit.ptr)
        self.tell(fit.ptr, stream)
