"""Fitting a ``DevicePolicy`` to labelled observations on the device: the ctypes binding of ``bsk_fit_*`` (include/bskgpu.h).

``PolicyFit`` attaches to one policy.  ``accumulate`` adds the gradient of a cross-entropy against int32 labels - and, with value
targets, of a squared error of the value network - over a batch of observations that is already in device memory; ``step`` is one
Adam update of a float64 master copy of the parameters, written back into the policy's own device block.  Everything between the
two is enqueued on one stream with no copy and no synchronisation, so a planner's ``d_best_action`` can be the labels with no host
in between (``planning.distill``) and the pair can be captured into a HIP graph.  The arithmetic is a fixed order of float32 fused
multiply-adds and float64 sums; ``policy_ref`` restates it (``fit_backward_ref``, ``fit_accumulate_ref``, ``fit_step_ref``).
Reached as ``basilisk_env_amd.policy.PolicyFit``."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .policy_base import _DeviceObject, _host_block
from .policy_ref import FIT_STATS_COLUMNS, check_fit, check_fit_batch
from .policy_spec import n_params


def _pointer(x, typestrs, what):
    """A raw device pointer, or anything with ``__cuda_array_interface__`` of one of ``typestrs`` -> (pointer, element count or
    None, shape or None); None stays None"""
    if x is None:
        return None, None, None
    cai = getattr(x, "__cuda_array_interface__", None)
    if cai is None:
        return int(x), None, None
    if cai["typestr"] not in typestrs:
        raise ValueError("%s: a device array of %s, got %r" % (what, " / ".join(typestrs), cai["typestr"]))
    shape = tuple(cai["shape"])
    return int(cai["data"][0]), int(np.prod(shape)) if shape else 1, shape


class PolicyFit(_DeviceObject):
    """A supervised fit of ``policy`` (a ``DevicePolicy``) on its GPU: ``lr`` and Adam's ``beta1``, ``beta2``, ``eps`` with the L2
    penalty ``weight_decay`` (``check_adam``'s rules), and ``value_coef``, the weight of the value network's squared error.  The
    master copy theta starts as the policy's parameters; every ``step`` writes float32(theta) back into the policy, whose ``act``
    and rollouts then run the fitted network with no further call.  ``policy.set_params`` does NOT reach theta: follow it with
    ``set_state(theta=...)``.  The policy must stay open while the fit is.  Not thread-safe, one stream at a time."""
    _kind, _what = "fit", "policy fit"

    def __init__(self, policy, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, value_coef=0.5):
        args = check_fit(lr, beta1, beta2, eps, weight_decay, value_coef)          # (before the handle exists: a bad one leaves none)
        self.policy = policy
        self.n_params = n_params(policy.spec)
        self._lr, self.adam, self.value_coef = args[0], args[1:5], args[5]
        self._lib = _lib.load()
        self.device = policy.device
        h = C.c_void_p()
        check(self._lib.bsk_fit_create(policy._handle(), *args, C.byref(h)))
        self._p = h
        self._out = self._source = None
        self._kept = ()

    def close(self):
        super(PolicyFit, self).close()
        self._kept = ()

    # ------------------------------------------------------------------ the two launches
    def accumulate(self, obs, labels, value_targets=None, alive=None, dlogits=None, n=None, stride=None, stream=0):
        """The gradient of one batch into the accumulators: two launches on ``stream``, no copy, no synchronisation; capturable once
        a batch of at least this size has been accumulated outside a capture.  ``obs``: a device array (5, n) float64 with
        contiguous rows, or a raw pointer to f64[5][stride] with ``n`` (``stride`` defaults to n).  ``labels``: int32 (n,) - a
        planner's ``d_best_action`` as it is; ``value_targets``: float64 (n,) or None (the value network is then left alone);
        ``alive``: n bytes or None, a zero byte takes the sample out, as a label outside 0..2 does; ``dlogits``: float32 (3, n)
        the output deltas are also written to, or None.  Each a raw device pointer or anything with
        ``__cuda_array_interface__``; arrays are kept alive until the next call."""
        cai = getattr(obs, "__cuda_array_interface__", None)
        if cai is not None:
            shape, strides = tuple(cai["shape"]), cai.get("strides")
            if cai["typestr"] != "<f8" or len(shape) != 2 or shape[0] != 5 or shape[1] < 1:
                raise ValueError("observations: a float64 device array of shape (5, n), got %r %r" % (cai["typestr"], shape))
            strides = (shape[1] * 8, 8) if strides is None else tuple(strides)
            if strides[1] != 8 or strides[0] % 8 or strides[0] < shape[1] * 8:
                raise ValueError("observations: rows must be contiguous and at least n elements apart")
            obs_ptr, n, stride = int(cai["data"][0]), shape[1], strides[0] // 8
        elif n is None:
            raise ValueError("a raw observation pointer needs n")
        else:
            obs_ptr = int(obs)
        stride = int(n) if stride is None else int(stride)
        lab, lab_n, _ = _pointer(labels, ("<i4",), "labels")
        tgt, tgt_n, _ = _pointer(value_targets, ("<f8",), "value targets")
        liv, liv_n, _ = _pointer(alive, ("|u1", "|b1"), "alive")
        dl, _, dl_shape = _pointer(dlogits, ("<f4",), "dlogits")
        n = check_fit_batch(self.policy.spec, n, lab_n, tgt_n if tgt_n is not None else (n if tgt else None), liv_n)
        if lab is None:
            raise ValueError("labels are required")
        if dl_shape is not None and dl_shape != (3, n):
            raise ValueError("dlogits: a float32 device array of shape (3, %d), got %r" % (n, dl_shape))
        vp = lambda p: C.c_void_p(p) if p else None      # noqa: E731
        handle = self._handle()
        self._kept = (obs, labels, value_targets, alive, dlogits)          # (the launches read them after this call returns)
        check(self._lib.bsk_fit_accumulate(handle, vp(obs_ptr), stride, n, vp(lab), vp(tgt), vp(liv), vp(dl), n,
                                           C.c_void_p(int(stream or 0))))

    def step(self, stream=0):
        """One Adam step of the mean gradient since the last one, then float32(theta) into the policy: three launches on
        ``stream``, no copy, no synchronisation, capturable.  Nothing moves when no sample has contributed."""
        check(self._lib.bsk_fit_step(self._handle(), C.c_void_p(int(stream or 0))))

    # ------------------------------------------------------------------ what it holds
    def stats_ptr(self):
        """The diagnostics row of the last ``accumulate`` as a DEVICE pointer to 4 float64, valid until ``close``."""
        p = C.c_void_p()
        check(self._lib.bsk_fit_stats_device(self._handle(), C.byref(p)))
        return p.value

    def stats(self):
        """The last ``accumulate``'s row -> dict by ``FIT_STATS_COLUMNS``: ``nll_sum`` (the summed cross-entropy), ``value_loss_sum``
        (the summed 0.5 (v - target)^2), ``correct`` (samples whose greedy action is the label) and ``count`` (samples that
        contributed).  A host read: synchronises."""
        from . import _hip
        row = np.empty(4, np.float64)
        self.sync()                                # (everything queued has written the row)
        with _hip.device_guard(self.device):
            _hip.check(_hip.runtime().hipMemcpyAsync(C.c_void_p(row.ctypes.data), C.c_void_p(self.stats_ptr()), row.nbytes,
                                                     _hip.hipMemcpyDeviceToHost, None), "hipMemcpyAsync")
        self.sync()
        return dict(zip(FIT_STATS_COLUMNS, (row[0], row[1], int(row[2]), int(row[3]))))

    def state(self):
        """-> dict ``theta``, ``m``, ``v`` float64 (n_params,), ``beta_pow`` float64 (2,) and ``steps``; synchronises."""
        out = {k: np.empty(self.n_params, np.float64) for k in ("theta", "m", "v")}
        out["beta_pow"] = np.empty(2, np.float64)
        steps = C.c_uint64()
        check(self._lib.bsk_fit_get_state(self._handle(), out["theta"].ctypes.data, out["m"].ctypes.data, out["v"].ctypes.data,
                                          out["beta_pow"].ctypes.data, C.byref(steps)))
        out["steps"] = steps.value
        return out

    def set_state(self, theta=None, m=None, v=None, beta_pow=None, steps=0):
        """``state()``'s arrays back (None keeps; ``steps`` always): a checkpoint resumes bit for bit.  A ``theta`` is also written
        to the policy as float32 - the way to give policy and fit new parameters together.  What has been accumulated since the
        last ``step`` is discarded (the accumulators are not part of ``state()``: take a checkpoint behind a step).  Synchronises."""
        arrs = [None if a is None else _host_block(a, size, np.float64, what="values")
                for a, size in ((theta, self.n_params), (m, self.n_params), (v, self.n_params), (beta_pow, 2))]
        check(self._lib.bsk_fit_set_state(self._handle(), *[None if a is None else a.ctypes.data for a in arrs], int(steps)))

    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, value):
        value = check_fit(value, *self.adam, self.value_coef)[0]
        check(self._lib.bsk_fit_set_lr(self._handle(), value))
        self._lr = value
