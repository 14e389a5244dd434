"""The argument rules of a policy and the layout of its parameter block (``bsk_policy_spec`` and the block of include/bskgpu.h).

``check_spec`` turns hidden widths and activations into a ``Spec`` or says what is wrong with them; ``layer_shapes``, ``n_params``,
``pack_params`` and ``unpack_params`` lay the block out - ``in_scale[5]``, ``in_shift[5]``, then ``W[out][in]`` and ``b[out]`` per layer,
the action network first - and ``torch_layers`` reads one network out of an ``nn.Sequential``.  ``check_sigma_adaptation`` holds the
argument rules of the evolution strategy's per-parameter step size, ``OUTCOME_COLUMNS`` names the columns of an episode-outcome
row and ``check_outcome_log`` holds the argument rule of the ring that keeps them.  Nothing here needs a device or the library: only its constants
and the mirror of the C struct are imported.
"""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

from ._lib import BSK_ABI_VERSION, BSK_OUTCOME_COLS, POLICY_GREEDY, POLICY_RELU, POLICY_SAMPLE, POLICY_TANH, BskPolicySpec

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
    c.abi_version, c.struct_size = BSK_ABI_VERSION, C.sizeof(BskPolicySpec)
    c.n_hidden, c.activation = len(spec.hidden), ACTIVATIONS[spec.activation]
    for k, w in enumerate(spec.hidden):
        c.hidden[k] = w
    if spec.value_hidden is not None:
        c.has_value, c.v_n_hidden, c.v_activation = 1, len(spec.value_hidden), ACTIVATIONS[spec.value_activation]
        for k, w in enumerate(spec.value_hidden):
            c.v_hidden[k] = w
    return c


def check_sigma_adaptation(lr_sigma, max_change, sigma_min, sigma_max, sigma=None):
    """The argument rules of ``bsk_es_set_sigma_adaptation(BSK_ES_SIGMA_PGPE, ...)`` -> the four as floats; ValueError where it
    returns BSK_EINVAL.  ``sigma``: the sigma the optimiser was created with (None: that rule is not checked).  Needs no device."""
    lr_sigma, max_change, sigma_min, sigma_max = (float(x) for x in (lr_sigma, max_change, sigma_min, sigma_max))
    if not math.isfinite(lr_sigma) or lr_sigma < 0.0:
        raise ValueError("lr_sigma must be finite and not negative")
    if not math.isfinite(max_change) or not (0.0 < max_change < 1.0):
        raise ValueError("max_change must be inside (0, 1)")
    if not math.isfinite(sigma_min) or not (sigma_min > 0.0):
        raise ValueError("sigma_min must be finite and positive")
    if not math.isfinite(sigma_max) or sigma_max < sigma_min:
        raise ValueError("sigma_max must be finite and not below sigma_min")
    if sigma is not None and not (sigma_min <= float(sigma) <= sigma_max):
        raise ValueError("the optimiser's sigma must be inside [sigma_min, sigma_max]")
    return lr_sigma, max_change, sigma_min, sigma_max


#: the columns of one member's episode-outcome row (``BSK_OUTCOME_COLS`` doubles; include/bskgpu.h, bsk_population_set_outcomes)
OUTCOME_COLUMNS = ("end_length", "end_wheels", "end_battery", "end_orbit", "unfinished", "steps_action0", "steps_action1",
                   "steps_action2", "value_sum_sq", "value_min", "value_max")
OUTCOME_COLS = BSK_OUTCOME_COLS
assert len(OUTCOME_COLUMNS) == OUTCOME_COLS                  # (one name per column of the header's row)


def check_outcome_log(capacity):
    """The argument rule of ``set_outcome_log`` -> the capacity as an int; ValueError where ``bsk_es_set_outcome_log`` returns
    BSK_EINVAL (0 turns the ring off).  Needs no device."""
    if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)):
        raise ValueError("outcome log capacity must be an integer, got %r" % (capacity,))
    if capacity < 0 or capacity > 2 ** 31 - 1:
        raise ValueError("outcome log capacity must be in 0..2^31-1, got %d" % capacity)
    return int(capacity)


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
