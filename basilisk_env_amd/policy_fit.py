"""Training a ``DevicePolicy`` on the device: the ctypes binding of ``bsk_fit_*`` and of the launches of a policy-gradient loop
(include/bskgpu.h).  Everything is enqueued on one stream with no copy, no synchronisation and no allocation, so it can be captured
into a HIP graph; every kernel's arithmetic is restated bit for bit in ``policy_ref``.  Reached as ``basilisk_env_amd.policy.<name>``.
In the file's order:

- ``_pointer`` / ``_arg``: how every device-buffer argument is read - a raw pointer or anything with ``__cuda_array_interface__``.
- ``PolicyFit``: gradients into accumulators and Adam on a float64 master copy.  ``accumulate`` (``bsk_fit_accumulate``: cross-entropy
  against labels, squared value error), ``accumulate_pg`` (``bsk_fit_accumulate_pg``: the clipped surrogate and an entropy bonus),
  ``accumulate_ppo`` (``bsk_fit_accumulate_ppo``: PPO2's clipped value loss besides), ``step`` (``bsk_fit_step``, under
  ``max_grad_norm`` with the clip of the global norm), ``apply_obs_norm``; the diagnostics rows (``bsk_fit_*_device``) and their host
  readers; ``state`` / ``set_state``; the schedule words (``bsk_fit_set_schedule``, ``bsk_fit_schedule_begin`` / ``_end``) and the KL
  stop (``bsk_fit_kl_gate``).
- the launches of the loop, one function each: ``gae`` (``bsk_gae``), ``normalize_advantages`` (``bsk_adv_normalize``),
  ``reward_normalize`` (``bsk_reward_norm``), ``pg_gather`` / ``pg_shuffle_advance`` (``bsk_pg_gather``, ``bsk_pg_shuffle_advance``: a
  minibatch by a permutation of two device words) and ``pg_episodes`` / ``pg_log_update`` / ``pg_log_advance`` (``bsk_pg_*``: one row
  of the training log per iteration).
- ``PolicyGradient``: the loop made of them - ``collect`` (rollout, values, advantages), ``update`` (``epoch``s of minibatch steps),
  ``iterate`` - and the host readers of its device state, for logs and checkpoints."""
import ctypes as C

import numpy as np

from . import _hip, _lib
from ._lib import check
from .policy_base import _DeviceObject, _host_block
from .policy_ref import (FIT_STATS_COLUMNS, PG_STATS_COLUMNS, VCLIP_STATS_COLUMNS, adv_normalize_work_bytes, check_adv_normalize,
                         check_fit, check_fit_batch, check_gae, check_max_grad_norm, check_pg, check_pg_episodes, check_pg_gather,
                         check_pg_log, check_pg_loop, check_pg_shuffle, check_reward_norm, PG_LOG_COLS, pg_episodes_work_bytes,
                         pg_log_table_ref, REWARD_NORM_STATE_WORDS, reward_norm_divisor, reward_norm_state_words,
                         reward_norm_work_bytes, check_pg_schedule, SCHED_LOG_COLUMNS, SCHED_STATE_FIELDS, SCHED_WORDS,
                         sched_log_table_ref)
from .policy_spec import n_params

_F8, _F4, _I4, _U1, _W64 = ("<f8",), ("<f4",), ("<i4",), ("|u1", "|b1"), ("<u8", "<i8")


def _vp(p):
    return C.c_void_p(p) if p else None


def _stream(stream):
    return C.c_void_p(int(stream or 0))


def _check_int(name, x, lo, hi, text):
    """``x`` as an int when it is an integer - not a bool - in lo .. hi (``hi`` None: no upper bound); ``text`` words the range"""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or int(x) < lo or (hi is not None and int(x) > hi):
        raise ValueError("%s must be an integer %s, got %r" % (name, text, x))
    return int(x)


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


def _arg(x, typestrs, what, need, must=False, in_bytes=False, text=None):
    """One device-buffer argument of a launch -> its ``c_void_p``, or None for a null pointer.  ``x`` as ``_pointer`` reads it; an
    array must hold at least ``need`` elements - bytes with ``in_bytes``, whatever its element type - and with ``must`` a null
    pointer is refused.  ``text`` replaces the wording of both refusals."""
    ptr, size, _ = _pointer(x, typestrs, what)
    if must and not ptr:
        raise ValueError(text or "%s: a device buffer is required" % what)
    if size is not None and in_bytes:
        size *= int(x.__cuda_array_interface__["typestr"][2:])
    if size is not None and size < need:
        raise ValueError(text or "%s: at least %d elements, got %d" % (what, need, size))
    return C.c_void_p(ptr) if ptr else None


class PolicyFit(_DeviceObject):
    """A supervised fit of ``policy`` (a ``DevicePolicy``) on its GPU: ``lr`` and Adam's ``beta1``, ``beta2``, ``eps`` with the L2
    penalty ``weight_decay`` (``check_adam``'s rules), ``value_coef``, the weight of the value network's squared error, and
    ``max_grad_norm``, the bound every ``step`` holds the global norm of the mean gradient to (0, the default: none).  The
    master copy theta starts as the policy's parameters; every ``step`` writes float32(theta) back into the policy, whose ``act``
    and rollouts then run the fitted network with no further call.  ``policy.set_params`` does NOT reach theta: follow it with
    ``set_state(theta=...)``.  The policy must stay open while the fit is.  Not thread-safe, one stream at a time."""
    _kind, _what = "fit", "policy fit"

    def __init__(self, policy, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, value_coef=0.5, max_grad_norm=0.0):
        args = check_fit(lr, beta1, beta2, eps, weight_decay, value_coef)          # (before the handle exists: a bad one leaves none)
        max_grad_norm = check_max_grad_norm(max_grad_norm)
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
        self._max_grad_norm = 0.0
        self._schedule = None
        if max_grad_norm:
            self.max_grad_norm = max_grad_norm

    def close(self):
        super(PolicyFit, self).close()
        self._kept = ()

    # ------------------------------------------------------------------ the launches
    def accumulate(self, obs, labels, value_targets=None, alive=None, dlogits=None, n=None, stride=None, stream=0):
        """The gradient of one batch into the accumulators: two launches on ``stream``, no copy, no synchronisation; capturable once
        a batch of at least this size has been accumulated outside a capture.  ``obs``: a device array (5, n) float64 with
        contiguous rows, or a raw pointer to f64[5][stride] with ``n`` (``stride`` defaults to n).  ``labels``: int32 (n,) - a
        planner's ``d_best_action`` as it is; ``value_targets``: float64 (n,) or None (the value network is then left alone);
        ``alive``: n bytes or None, a zero byte takes the sample out, as a label outside 0..2 does; ``dlogits``: float32 (3, n)
        the output deltas are also written to, or None.  Each a raw device pointer or anything with
        ``__cuda_array_interface__``; arrays are kept alive until the next call."""
        obs_ptr, stride, n, lab, tgt, liv, dl = self._batch(obs, labels, value_targets, alive, dlogits, n, stride, "labels")
        handle = self._handle()
        self._kept = (obs, labels, value_targets, alive, dlogits)          # (the launches read them after this call returns)
        check(self._lib.bsk_fit_accumulate(handle, _vp(obs_ptr), stride, n, _vp(lab), _vp(tgt), _vp(liv), _vp(dl), n, _stream(stream)))

    def _batch(self, obs, labels, value_targets, alive, dlogits, n, stride, noun):
        """The pointer and array rules of ``accumulate`` -> (obs pointer, stride, n, labels, targets, alive, dlogits pointers)"""
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
        lab, lab_n, _ = _pointer(labels, _I4, noun)
        tgt, tgt_n, _ = _pointer(value_targets, _F8, "value targets")
        liv, liv_n, _ = _pointer(alive, _U1, "alive")
        dl, _, dl_shape = _pointer(dlogits, _F4, "dlogits")
        n = check_fit_batch(self.policy.spec, n, lab_n, tgt_n if tgt_n is not None else (n if tgt else None), liv_n)
        if lab is None:
            raise ValueError("%s are required" % noun)
        if dl_shape is not None and dl_shape != (3, n):
            raise ValueError("dlogits: a float32 device array of shape (3, %d), got %r" % (n, dl_shape))
        return obs_ptr, stride, n, lab, tgt, liv, dl

    def _pg_batch(self, obs, actions, advantages, logp_old, clip, ent_coef, value_targets, alive, dlogits, n, stride, more=()):
        """``_batch`` and the rules ``accumulate_pg`` adds -> (``_batch``'s seven, clip, ent_coef, the pointers of advantages, old
        log-probabilities and of every (noun, float32 (n,) array) of ``more``)"""
        batch = self._batch(obs, actions, value_targets, alive, dlogits, n, stride, "actions")
        named = (("advantages", advantages), ("old log-probabilities", logp_old)) + more
        read = [_pointer(x, _F4, what) for what, x in named]
        if read[0][0] is None:
            raise ValueError("advantages are required")
        for (what, _), (_, size, _) in zip(named, read):
            if size is not None and size != batch[2]:
                raise ValueError("%s: %d elements, got %d" % (what, batch[2], size))
        return batch + check_pg(clip, ent_coef, read[1][0] is not None) + ([ptr for ptr, _, _ in read],)

    def accumulate_pg(self, obs, actions, advantages, logp_old=None, clip=0.2, ent_coef=0.0, value_targets=None, alive=None,
                      dlogits=None, n=None, stride=None, stream=0):
        """``accumulate`` with the policy-gradient output deltas (``bsk_fit_accumulate_pg``; three launches): ``actions`` int32 (n,) - the actions
        taken, in the labels' place -, ``advantages`` float32 (n,) and ``logp_old`` float32 (n,), the log-probabilities the actions
        were taken with, or None (A2C: no ratio, no clipping; ``clip`` is then not read).  ``ent_coef``: the weight of the entropy
        bonus.  Everything else, the pointer and array rules included, is ``accumulate``'s; ``pg_stats`` has the row it adds."""
        obs_ptr, stride, n, act, tgt, liv, dl, clip, ent_coef, (adv, old) = self._pg_batch(
            obs, actions, advantages, logp_old, clip, ent_coef, value_targets, alive, dlogits, n, stride)
        handle = self._handle()
        self._kept = (obs, actions, advantages, logp_old, value_targets, alive, dlogits)
        check(self._lib.bsk_fit_accumulate_pg(handle, _vp(obs_ptr), stride, n, _vp(act), _vp(adv), _vp(old), clip, ent_coef, _vp(tgt),
                                              _vp(liv), _vp(dl), n, _stream(stream)))

    def accumulate_ppo(self, obs, actions, advantages, logp_old=None, clip=0.2, ent_coef=0.0, value_targets=None, value_old=None,
                       clip_vf=None, alive=None, dlogits=None, dvalue=None, n=None, stride=None, stream=0):
        """``accumulate_pg`` with PPO2's clipped value loss (``bsk_fit_accumulate_ppo``): ``value_old`` float32 (n,) - the values
        the rollout recorded - with ``clip_vf`` finite and positive, or None (the plain squared error; ``clip_vf`` is then not
        read), and ``dvalue`` float32 (n,) or None, which receives the value network's output delta of every sample, the counterpart
        of ``dlogits``.  Either needs ``value_targets``.  With neither the launches are ``accumulate_pg``'s; ``vclip_stats`` has the
        row ``value_old`` adds.  Everything else, the pointer and array rules included, is ``accumulate_pg``'s."""
        obs_ptr, stride, n, act, tgt, liv, dl, clip, ent_coef, (adv, old, vold, dv) = self._pg_batch(
            obs, actions, advantages, logp_old, clip, ent_coef, value_targets, alive, dlogits, n, stride,
            (("old values", value_old), ("dvalue", dvalue)))
        if (vold is not None or dv is not None) and tgt is None:
            raise ValueError("old values and dvalue need value targets")
        if vold is None:
            clip_vf = 0.0                          # (not read)
        elif clip_vf is None:
            raise ValueError("clip_vf is required with old values")
        else:
            clip_vf = check_pg_shuffle(cliprange_vf=clip_vf)[2]
        handle = self._handle()
        self._kept = (obs, actions, advantages, logp_old, value_targets, value_old, alive, dlogits, dvalue)
        check(self._lib.bsk_fit_accumulate_ppo(handle, _vp(obs_ptr), stride, n, _vp(act), _vp(adv), _vp(old), clip, ent_coef, _vp(tgt),
                                               _vp(vold), clip_vf, _vp(liv), _vp(dl), n, _vp(dv), _stream(stream)))

    def step(self, stream=0):
        """One Adam step of the mean gradient since the last one, then float32(theta) into the policy: three launches on
        ``stream`` - four with ``max_grad_norm`` set, the gradient's global norm in front -, no copy, no synchronisation,
        capturable.  Nothing moves when no sample has contributed."""
        check(self._lib.bsk_fit_step(self._handle(), _stream(stream)))

    def apply_obs_norm(self, stats, std_min=1e-6, stream=0):
        """in_scale / in_shift out of an ``ObsStats`` (``obs_norm_ref``) into theta[0:10] - which no step moves - and float32(theta)
        into the policy (``bsk_fit_apply_obs_norm``): two launches on ``stream``, no copy, no synchronisation, capturable.  While
        nothing has been counted theta keeps what it has; theta[10:], m and v are never touched."""
        check(self._lib.bsk_fit_apply_obs_norm(self._handle(), stats._handle(), float(std_min), _stream(stream)))

    # ------------------------------------------------------------------ what it holds
    def _device_words(self, name):
        """``bsk_fit_<name>_device``: the DEVICE pointer to words of the fit"""
        p = C.c_void_p()
        check(self._c(name + "_device")(self._handle(), C.byref(p)))
        return p.value

    def stats_ptr(self):
        """The diagnostics row of the last ``accumulate`` as a DEVICE pointer to 4 float64, valid until ``close``."""
        return self._device_words("stats")

    def pg_stats_ptr(self):
        """The policy-gradient row of the last ``accumulate_pg`` as a DEVICE pointer to 4 float64, valid until ``close``."""
        return self._device_words("pg_stats")

    def vclip_stats_ptr(self):
        """The value-clip row of the last ``accumulate_ppo`` with ``value_old`` as a DEVICE pointer to 2 float64, valid until
        ``close``."""
        return self._device_words("vclip_stats")

    def grad_norm_ptr(self):
        """{norm, scale} of the last ``step`` taken with ``max_grad_norm`` set as a DEVICE pointer to 2 float64, valid until
        ``close``."""
        return self._device_words("grad_norm")

    def schedule_ptr(self):
        """The eight schedule words (``SCHED_STATE_FIELDS``) as a DEVICE pointer, valid until ``close``."""
        return self._device_words("schedule")

    def _row(self, ptr, words=4):
        row = np.empty(words, np.float64)
        self.sync()                                # (everything queued has written the row)
        with _hip.device_guard(self.device):
            _hip.check(_hip.runtime().hipMemcpyAsync(C.c_void_p(row.ctypes.data), C.c_void_p(ptr), row.nbytes,
                                                     _hip.hipMemcpyDeviceToHost, None), "hipMemcpyAsync")
        self.sync()
        return row

    def stats(self):
        """The last ``accumulate``'s row -> dict by ``FIT_STATS_COLUMNS``: ``nll_sum`` (the summed cross-entropy), ``value_loss_sum``
        (the summed 0.5 (v - target)^2), ``correct`` (samples whose greedy action is the label) and ``count`` (samples that
        contributed).  A host read: synchronises."""
        row = self._row(self.stats_ptr())
        return dict(zip(FIT_STATS_COLUMNS, (row[0], row[1], int(row[2]), int(row[3]))))

    def pg_stats(self):
        """The last ``accumulate_pg``'s row -> dict by ``PG_STATS_COLUMNS``: ``kl_sum`` (the summed old minus new log-probability of
        the actions taken, an estimate of the KL divergence from the old policy; 0 without ``logp_old``), ``entropy_sum``,
        ``clipped`` (samples whose ratio left the clip range on the side that zeroes their gradient) and ``surrogate_sum`` (the
        summed advantage times ratio).  A host read: synchronises."""
        row = self._row(self.pg_stats_ptr())
        return dict(zip(PG_STATS_COLUMNS, (row[0], row[1], int(row[2]), row[3])))

    def vclip_stats(self):
        """The last ``accumulate_ppo`` with ``value_old``'s row -> dict by ``VCLIP_STATS_COLUMNS``: ``value_clipped`` (samples whose
        clipped branch held the max, and whose value gradient is therefore zero) and ``value_loss_unclipped_sum`` (the summed
        0.5 (v - target)^2, whatever the branch).  A host read: synchronises."""
        row = self._row(self.vclip_stats_ptr(), 2)
        return dict(zip(VCLIP_STATS_COLUMNS, (int(row[0]), row[1])))

    def grad_norm(self):
        """-> dict ``norm`` (the global norm of the last clipped step's mean gradient, before clipping) and ``scale`` (what the
        step multiplied it by: exactly 1.0 while the norm was within ``max_grad_norm``); (0.0, 1.0) before the first.  A host read:
        synchronises."""
        row = self._row(self.grad_norm_ptr(), 2)
        return {"norm": float(row[0]), "scale": float(row[1])}

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

    # ------------------------------------------------------------------ schedules and the KL stop
    def set_schedule(self, total, lr, clip, clip_vf, ent_coef, kl_stop=0.0):
        """Attaches a schedule (``bsk_fit_set_schedule``): each of ``lr``, ``clip``, ``clip_vf`` and ``ent_coef`` a pair (a, b) - a at
        iteration 0, b from iteration ``total`` on, a line between (``policy_ref.pg_schedule_ref``; ``total`` = 0: a for ever) -
        and ``kl_stop``, 0 (none) or the mean KL of a minibatch above which ``kl_gate`` drops the rest of an update.  From here on
        ``accumulate_pg`` / ``accumulate_ppo`` and ``step`` read the values from eight device words of the fit and not from their
        arguments (which are still checked) or ``lr``, so a captured graph trains at what the words hold at each replay.  The words
        start at iteration 0.  Synchronises."""
        total, lr, clip, clip_vf, ent_coef, kl_stop = check_pg_schedule(total, lr, clip, clip_vf, ent_coef, kl_stop)
        sc = _lib.BskFitSchedule((C.c_double * 2)(*lr), (C.c_double * 2)(*clip), (C.c_double * 2)(*clip_vf), (C.c_double * 2)(*ent_coef),
                                 total, kl_stop)
        check(self._lib.bsk_fit_set_schedule(self._handle(), C.byref(sc)))
        self._schedule = (total, lr, clip, clip_vf, ent_coef, kl_stop)

    def clear_schedule(self):
        """Detaches the schedule: the launches and arguments of a fit that never had one."""
        check(self._lib.bsk_fit_set_schedule(self._handle(), None))
        self._schedule = None

    @property
    def schedule(self):
        """(total, lr, clip, clip_vf, ent_coef, kl_stop) as attached, the four as pairs, or None."""
        return self._schedule

    def schedule_begin(self, stream=0):
        """``bsk_fit_schedule_begin``: lr, clip, clip_vf and ent_coef of the iteration the words hold, the gate open - one launch on
        ``stream``, no copy, no synchronisation, capturable."""
        check(self._lib.bsk_fit_schedule_begin(self._handle(), _stream(stream)))

    def kl_gate(self, diag, n_rows, stream=0):
        """``bsk_fit_kl_gate`` over ``diag`` float64 [n_rows][8] - the loop's ``log`` rows of the accumulates since the last step -,
        in front of ``step``: once their mean KL is not <= ``kl_stop`` (or the gate is closed already) what has been accumulated is
        dropped, and ``step`` moves nothing.  One launch on ``stream``, no copy, no synchronisation, capturable
        (``policy_ref.fit_kl_gate_ref``)."""
        _pointer(diag, _F8, "diag")                # (its element type is looked at before n_rows)
        n_rows = _check_int("n_rows", n_rows, 1, None, ">= 1")
        diag = _arg(diag, _F8, "diag", 8 * n_rows, True, text="diag: a device buffer of at least %d float64" % (8 * n_rows))
        check(self._lib.bsk_fit_kl_gate(self._handle(), diag, n_rows, _stream(stream)))

    def schedule_end(self, ring=None, capacity=0, stream=0):
        """``bsk_fit_schedule_end``: with ``ring`` float64 [capacity][8] the iteration's row of ``SCHED_LOG_COLUMNS`` into slot
        iteration % capacity; then iteration += 1.  One launch on ``stream``, no copy, no synchronisation, capturable."""
        if _pointer(ring, _F8, "ring")[0]:
            capacity = _check_int("capacity", capacity, 1, 2 ** 31 - 1, "in 1 .. 2^31 - 1 with a ring")
            ring = _arg(ring, _F8, "ring", 8 * capacity, text="ring: at least %d float64" % (8 * capacity))
        else:
            ring, capacity = None, 0
        check(self._lib.bsk_fit_schedule_end(self._handle(), ring, capacity, _stream(stream)))

    def schedule_words(self):
        """The eight words as the device holds them -> uint64 (8,).  Synchronises."""
        words = np.empty(SCHED_WORDS, np.uint64)
        check(self._lib.bsk_fit_get_schedule_state(self._handle(), C.c_void_p(words.ctypes.data)))
        return words

    def schedule_state(self):
        """The eight words decoded -> dict by ``SCHED_STATE_FIELDS``: ``lr``, ``clip``, ``clip_vf``, ``ent_coef`` and ``kl_at_stop``
        floats, ``iteration``, ``gate`` and ``steps_skipped`` ints.  Synchronises."""
        words = self.schedule_words()
        f = words.view(np.float64)
        return {name: (float(f[k]) if k < 4 or k == 7 else int(words[k])) for k, name in enumerate(SCHED_STATE_FIELDS)}

    def set_schedule_state(self, iteration):
        """The iteration back, for checkpoints: the words of that iteration with the gate open, as ``schedule_begin`` would leave
        them.  Synchronises."""
        iteration = _check_int("iteration", iteration, 0, 2 ** 64 - 1, "in 0 .. 2^64 - 1")
        check(self._lib.bsk_fit_set_schedule_state(self._handle(), iteration))

    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, value):
        value = check_fit(value, *self.adam, self.value_coef)[0]
        check(self._lib.bsk_fit_set_lr(self._handle(), value))
        self._lr = value

    @property
    def max_grad_norm(self):
        """The bound on the global norm of the mean gradient a ``step`` enforces (``bsk_fit_set_max_grad_norm``; PPO2: 0.5), or 0:
        no clip, and ``step`` launches what it launches without one."""
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        value = check_max_grad_norm(value)
        check(self._lib.bsk_fit_set_max_grad_norm(self._handle(), value))
        self._max_grad_norm = value


def gae(reward_hist, reason_hist, value_hist, last_value, n_steps, n_envs, adv, ret=None, gamma=0.99, lam=0.95, stride=None, stream=0):
    """``bsk_gae``: generalised advantage estimation over the histories of a rollout, one launch on ``stream`` of the current device,
    no copy, no synchronisation, no allocation.  Each array a raw device pointer or anything with ``__cuda_array_interface__``:
    ``reward_hist`` float64, ``reason_hist`` uint8 and ``value_hist`` float32 [n_steps][stride] (``stride`` defaults to
    ``n_envs``), ``last_value`` float32 [n_envs] or None (= 0), ``adv`` float32 and ``ret`` float64 (or None) [n_steps][stride].
    Every non-zero reason byte - the time limit included - ends the episode for the estimator (``policy_ref.gae_ref``)."""
    n_steps, n_envs, stride, gamma, lam = check_gae(n_steps, n_envs, n_envs if stride is None else stride, gamma, lam)
    N = n_steps * stride
    reward, reason = _arg(reward_hist, _F8, "reward history", N), _arg(reason_hist, _U1, "reason history", N)
    value, last = _arg(value_hist, _F4, "value history", N), _arg(last_value, _F4, "last value", n_envs)
    adv, ret = _arg(adv, _F4, "advantages", N), _arg(ret, _F8, "returns", N)
    check(_lib.load().bsk_gae(reward, reason, value, last, n_steps, n_envs, stride, gamma, lam, adv, ret, _stream(stream)))


def normalize_advantages(adv, rows, n, out=None, alive=None, eps=1e-8, stride=None, work=None, stream=0):
    """``bsk_adv_normalize``: (A - mean) / (sd + eps) over the block ``adv`` float32 [rows][stride] (``stride`` defaults to ``n``)
    - the rows of one minibatch - into ``out`` (None: in place); ``alive`` uint8 [rows][stride] or None (every sample counts;
    a sample that does not count becomes 0).  ``work``: a device buffer of ``adv_normalize_work_bytes(n)`` bytes, whose first four
    float64 are afterwards mean, sd, 1 / (sd + eps) and the number of samples.  Each a raw device pointer or anything with
    ``__cuda_array_interface__``.  Three launches on ``stream`` of the current device, no copy, no synchronisation, no allocation
    (``policy_ref.adv_normalize_ref``, equal bit for bit)."""
    rows, n, stride, eps = check_adv_normalize(rows, n, n if stride is None else stride, eps)
    if work is None:
        raise ValueError("work: a device buffer of adv_normalize_work_bytes(n) bytes is required")
    N = rows * stride
    src, alive = _arg(adv, _F4, "advantages", N), _arg(alive, _U1, "alive", N)
    out = _arg(adv if out is None else out, _F4, "out", N)
    work = _arg(work, ("<f8", "|u1", "<u8"), "work", adv_normalize_work_bytes(n), in_bytes=True)
    check(_lib.load().bsk_adv_normalize(src, alive, rows, n, stride, eps, out, work, _stream(stream)))


def reward_normalize(reward_hist, reason_hist, n_steps, n_envs, state, out=None, ret_run=None, work=None, gamma=0.99, eps=1e-8,
                     clip=10.0, update=True, stride=None, stream=0):
    """``bsk_reward_norm``: the rewards ``reward_hist`` float64 [n_steps][stride] (``stride`` defaults to ``n_envs``) divided by the
    running standard deviation of the discounted return and clipped to [-clip, clip], into ``out`` (None: in place) -
    VecNormalize(norm_reward=True) for a whole rollout.  ``state``: ``REWARD_NORM_STATE_WORDS`` = 8 device words of 8 bytes, all
    zero when fresh, carried from call to call; ``ret_run`` float64 [n_envs]: every env's running discounted return, carried
    likewise; ``reason_hist`` uint8 [n_steps][stride]: a non-zero byte ends the env's return; ``work``:
    ``reward_norm_work_bytes(n_envs)`` bytes.  With ``update`` the statistics take in the WHOLE rollout first (two launches) and
    then the whole rollout is divided by the deviation that holds it (one launch); without it the statistics are frozen, only the
    last launch is made, and ``ret_run`` and ``work`` may be None.  Each a raw device pointer or anything with
    ``__cuda_array_interface__``.  On ``stream`` of the current device, no copy, no synchronisation, no allocation
    (``policy_ref.reward_norm_ref``, equal bit for bit)."""
    n_steps, n_envs, stride, gamma, eps, clip = check_reward_norm(n_steps, n_envs, n_envs if stride is None else stride, gamma, eps, clip)
    update = bool(update)
    N = n_steps * stride
    words = ("<f8", "|u1", "<u8", "<i8")
    reward, reason = _arg(reward_hist, _F8, "reward history", N, True), _arg(reason_hist, _U1, "reason history", N, True)
    ret_run = _arg(ret_run, _F8, "ret_run", n_envs, update)
    state = _arg(state, words, "state", 8 * REWARD_NORM_STATE_WORDS, True, in_bytes=True)
    work = _arg(work, words, "work", reward_norm_work_bytes(n_envs), update, in_bytes=True)
    out = _arg(reward_hist if out is None else out, _F8, "out", N, True)
    check(_lib.load().bsk_reward_norm(reward, reason, n_steps, n_envs, stride, gamma, eps, clip, int(update), ret_run, state, work, out,
                                      _stream(stream)))


def pg_gather(state, n_steps, n_envs, q0, m, obs_hist=None, action_hist=None, adv=None, logp_hist=None, ret=None, value_hist=None,
              obs_out=None, action_out=None, adv_out=None, logp_out=None, ret_out=None, value_out=None, index_out=None, stride=None,
              out_stride=None, stream=0):
    """``bsk_pg_gather``: one minibatch out of a rollout's histories into contiguous buffers, one launch on ``stream`` of the
    current device, no copy, no synchronisation, no allocation.  Output position i in [0, m) takes sample
    s = perm(q0 + i) of the n_steps * n_envs - the permutation of the two device words ``state`` = {seed, epoch}
    (``policy_ref.pg_perm_ref``) - or s = q0 + i with ``state`` None.  ``obs_hist`` float64 [n_steps][5][stride] -> ``obs_out``
    float64 [5][out_stride] (``out_stride`` defaults to m); ``action_hist`` int32, ``adv``, ``logp_hist``, ``value_hist`` float32 and
    ``ret`` float64 [n_steps][stride] (``stride`` defaults to ``n_envs``) -> their ``_out`` [m]; ``index_out`` int32 [m] receives s.
    A history and its output go together; each a raw device pointer or anything with ``__cuda_array_interface__``."""
    n_steps, n_envs, stride, q0, m, out_stride = check_pg_gather(n_steps, n_envs, n_envs if stride is None else stride, q0, m,
                                                                 m if out_stride is None else out_stride)
    N = n_steps * stride
    pairs = (("observations", obs_hist, obs_out, _F8, 5 * N, 4 * out_stride + m), ("actions", action_hist, action_out, _I4, N, m),
             ("advantages", adv, adv_out, _F4, N, m), ("log-probabilities", logp_hist, logp_out, _F4, N, m),
             ("returns", ret, ret_out, _F8, N, m), ("values", value_hist, value_out, _F4, N, m))
    src, dst = [], []
    for what, a, b, types, need_a, need_b in pairs:
        if (a is None) != (b is None):
            raise ValueError("%s: a history and its output are given together or not at all" % what)
        src.append(_arg(a, types, what, need_a))
        dst.append(_arg(b, types, what, need_b))
    idx = _arg(index_out, _I4, "index_out", m)
    if not idx and not any(src):
        raise ValueError("nothing to write")
    state = _arg(state, _W64, "state", 2, text="state: two 64-bit words {seed, epoch}")
    check(_lib.load().bsk_pg_gather(state, n_steps, n_envs, stride, q0, m, *src, dst[0], out_stride, *dst[1:], idx, _stream(stream)))


def pg_shuffle_advance(state, stream=0):
    """``bsk_pg_shuffle_advance``: epoch += 1 in the two device words ``state``, one launch on ``stream``, no copy, no
    synchronisation."""
    state = _arg(state, _W64, "state", 2, True, text="state: two 64-bit device words {seed, epoch}")
    check(_lib.load().bsk_pg_shuffle_advance(state, _stream(stream)))


def pg_episodes(reward_hist, reason_hist, n_steps, n_envs, ep_return, ep_len, work, ring, capacity, counter=None, action_hist=None,
                value_hist=None, ret=None, stride=None, stream=0):
    """``bsk_pg_episodes``: columns 0 .. 15 of a training-log row (``PG_LOG_COLUMNS``) out of one rollout's histories, two launches
    on ``stream`` of the current device, no copy, no synchronisation, no allocation.  ``reward_hist`` float64 and ``reason_hist``
    uint8 [n_steps][stride] (``stride`` defaults to ``n_envs``); ``action_hist`` int32 or None; ``value_hist`` float32 and ``ret``
    float64, both or neither (without them the explained variance is NaN).  ``ep_return`` float64 [n_envs] and ``ep_len`` int32
    [n_envs] carry every env's running episode from call to call (zeros: fresh envs); ``work``: ``pg_episodes_work_bytes(n_envs)``
    bytes; ``ring`` float64 [capacity][26], of which slot ``counter`` % capacity is written - ``counter`` one uint64 device word, or
    None: slot 0.  Each a raw device pointer or anything with ``__cuda_array_interface__`` (``policy_ref.pg_episodes_ref``, equal bit
    for bit)."""
    n_steps, n_envs, stride, capacity = check_pg_episodes(n_steps, n_envs, n_envs if stride is None else stride, capacity,
                                                          value_hist is not None, ret is not None)
    N = n_steps * stride
    reward, reason = _arg(reward_hist, _F8, "reward history", N, True), _arg(reason_hist, _U1, "reason history", N, True)
    action, value, ret = _arg(action_hist, _I4, "action history", N), _arg(value_hist, _F4, "value history", N), _arg(ret, _F8, "returns", N)
    ep_return, ep_len = _arg(ep_return, _F8, "ep_return", n_envs, True), _arg(ep_len, _I4, "ep_len", n_envs, True)
    work = _arg(work, ("<f8", "|u1", "<u8", "<i8"), "work", pg_episodes_work_bytes(n_envs), True, in_bytes=True)
    ring, counter = _arg(ring, _F8, "ring", capacity * PG_LOG_COLS, True), _arg(counter, _W64, "counter", 1)
    check(_lib.load().bsk_pg_episodes(reward, reason, action, value, ret, n_steps, n_envs, stride, ep_return, ep_len, work, ring, capacity,
                                      counter, _stream(stream)))


def pg_log_update(diag, n_rows, ring, capacity, counter=None, norms=None, n_norms=None, stream=0):
    """``bsk_pg_log_update``: columns 16 .. 25 of slot ``counter`` % capacity of ``ring`` (slot 0 with ``counter`` None) - the sum of
    the ``n_rows`` rows of ``diag`` float64 [n_rows][8], and of the ``n_norms`` {norm, scale} rows of ``norms`` float64 [n_norms][2]
    (or None) the sum of the norms and the number of rows with scale < 1.  One launch on ``stream``, no copy, no synchronisation
    (``policy_ref.pg_log_update_ref``)."""
    if norms is not None and n_norms is None:
        raise ValueError("n_norms: the number of {norm, scale} rows is required with norms")
    n_rows, capacity, n_norms = check_pg_log(n_rows, capacity, None if norms is None else n_norms)
    n_norms = n_norms or 0
    diag, norms = _arg(diag, _F8, "diag", 8 * n_rows, True), _arg(norms, _F8, "norms", 2 * n_norms)
    ring, counter = _arg(ring, _F8, "ring", capacity * PG_LOG_COLS, True), _arg(counter, _W64, "counter", 1)
    check(_lib.load().bsk_pg_log_update(diag, n_rows, norms, n_norms, ring, capacity, counter, _stream(stream)))


def pg_log_advance(gen, capacity, counter, stream=0):
    """``bsk_pg_log_advance``: gen[counter % capacity] = counter, counter += 1 - ``gen`` uint64 [capacity], ``counter`` one uint64
    device word.  One launch on ``stream``, no copy, no synchronisation."""
    _, capacity, _ = check_pg_log(1, capacity)
    gen = _arg(gen, _W64, "gen", capacity, True, text="gen: %d 64-bit device words" % capacity)
    counter = _arg(counter, _W64, "counter", 1, True, text="counter: 1 64-bit device words")
    check(_lib.load().bsk_pg_log_advance(gen, capacity, counter, _stream(stream)))


def _copy_row(dst, src, nbytes, stream):
    """``nbytes`` from one device address to another, enqueued on ``stream`` of the current device"""
    _hip.check(_hip.runtime().hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), nbytes, _hip.hipMemcpyDeviceToDevice, C.c_void_p(stream)),
               "hipMemcpyAsync")


class PolicyGradient(object):
    """On-device policy-gradient training (PPO; the clipped surrogate of ``bsk_fit_accumulate_pg`` on advantages from ``bsk_gae``):
    ``env`` - a ``BatchedPropagator`` (or an env over one) created with ``FLAG_AUTO_RESET`` -, ``policy`` - a ``DevicePolicy`` with a
    value network - and ``fit``, the ``PolicyFit`` attached to it.  ``iterate()`` is ``collect()`` - ``n_steps`` env steps of
    ``substeps`` under the sampled policy, then values and advantages - and ``update()`` - ``epochs`` passes over ``minibatches``
    groups of consecutive time rows, one ``accumulate_pg`` per row and one Adam step per group.  Everything is enqueued on the
    env's stream from buffers allocated here: neither allocates, copies to or from the host or synchronises; ``iterate`` waits
    once, at its end, for the log.  ``close()`` frees the buffers (not the env, the policy or the fit).

    PPO2's conditioning of the update, each off by default and leaving the launches above as they are when off:
    ``normalize_advantages`` - behind ``bsk_gae`` every minibatch's group of rows is normalised on its own (``bsk_adv_normalize``)
    into a second buffer ``adv_norm``, which ``update()`` then reads (``adv`` keeps the raw estimate; the groups are the same in every
    epoch); ``obs_stats`` - an ``ObsStats`` attached to the policy here and detached by ``close()``, fed by the rollouts, and turned
    into the policy's in_scale / in_shift (``fit.apply_obs_norm(obs_stats, std_min)``) at the START of ``collect()``, never between a
    rollout and its update, so that the first minibatch still sees ratio 1; and, when ``fit.max_grad_norm`` is set at the time of
    ``update()``, the {norm, scale} row of every step in ``grad_norms``, float64 (epochs * minibatches, 2), after ``iterate()``
    (None otherwise).

    And the rest of PPO2's update, off by default likewise.  ``shuffle`` - a minibatch is no longer a group of rows but
    M = (n_steps // minibatches) * n_envs samples of a permutation of ALL n_steps * n_envs, a new one in every epoch: per
    minibatch one ``pg_gather`` into contiguous buffers ``mb_*``, then the accumulates over chunks of ``n_envs`` of them, and
    behind every epoch ``pg_shuffle_advance``.  The permutation is a function of the two device words ``{seed, epoch}``
    (``shuffle_state`` / ``set_shuffle_state``; ``policy_ref.pg_perm_ref``), so a captured epoch draws a new one at every replay.
    ``normalize_advantages`` then normalises every gathered minibatch in place - PPO2's rule, over the random subset - and
    ``collect()`` normalises nothing.  ``cliprange_vf`` - the clipped value loss of ``PolicyFit.accumulate_ppo`` against the
    rollout's recorded values, with or without ``shuffle``.  ``PolicyGradient(shuffle=True, normalize_advantages=True,
    cliprange_vf=0.2)`` with ``fit.max_grad_norm = 0.5`` is PPO2's update.

    ``log_capacity`` > 0 keeps a training log of that many iterations on the device, as ``DeviceEvolutionStrategy`` does: a ring of
    rows of ``PG_LOG_COLUMNS`` - how many episodes ended in the rollout, their returns and lengths, how they ended, which actions
    were taken, PPO2's explained variance, and the update's diagnostics summed over the iteration.  ``collect()`` then ends with
    ``pg_episodes`` over its histories - the return and the length of every env's running episode are carried from rollout to
    rollout in ``ep_return`` / ``ep_len`` - and ``update()`` with ``pg_log_update`` and ``pg_log_advance``; ``training_log()`` reads
    the ring.  The rows survive the replay of a captured iteration, which overwrites ``log``.  Nothing in it writes what training
    reads: theta, m, v and the histories are the same bit for bit with the log on.  0, the default, allocates and enqueues what
    the loop always did.

    ``normalize_rewards`` - VecNormalize(norm_reward=True), off by default: between the value launch and ``bsk_gae``, ``collect()``
    enqueues ``reward_normalize`` (``bsk_reward_norm``) with the loop's ``gamma``, ``reward_eps`` and ``reward_clip``, out of
    ``reward`` into a second history ``reward_norm``, which ``bsk_gae`` then reads.  The statistics - eight device words
    ``reward_state`` - and every env's running discounted return ``ret_run`` are carried from rollout to rollout on the device, so
    a replayed graph keeps accumulating them.  Unlike VecNormalize, which updates step by step, the statistics take in the whole
    rollout first and the whole rollout is then divided by one number: the scale is defined in the first rollout.  ``reward``
    keeps the raw rewards and ``pg_episodes`` still reads those, so the training log reports true returns.
    ``update_reward_stats`` (an attribute, True) is read when ``collect()`` enqueues: set it to False to freeze the statistics, as
    for evaluation; a captured graph bakes in the value it was captured with.  ``reward_norm_state()`` /
    ``set_reward_norm_state()`` are for checkpoints and ``reward_scale()`` is the current divisor.  A value network trained this
    way is in units of reward / sd: the planners' ``bootstrap=`` adds its output to RAW rewards, so a caller that bootstraps from it
    must multiply the values by ``reward_scale()`` - nothing in the planners does.  Off, the loop allocates and enqueues what it
    always did: the same launches, the same arguments, the same buffers.

    Schedules and a KL stop, off by default: ``total_iterations`` with ``lr_end``, ``clip_end``, ``cliprange_vf_end`` and
    ``ent_coef_end`` (None: constant) anneals ``fit.lr``, ``clip``, ``cliprange_vf`` and ``ent_coef`` - as they are when the loop is
    created - linearly to their ends over that many ``update()`` calls (``policy_ref.pg_schedule_ref``; PPO2's annealing is an end of
    0 for lr), and ``kl_stop`` > 0 drops the remaining steps of an update once a minibatch's mean KL, the loop's estimator
    mean(logp_old - logp), is above it (``policy_ref.fit_kl_gate_ref``); ``kl_stop`` alone attaches a constant schedule.  The loop
    then attaches a schedule to the fit (``PolicyFit.set_schedule``; ``close()`` clears it) and ``update()`` enqueues
    ``schedule_begin`` in front, ``kl_gate`` over every minibatch's rows of ``log`` in front of its step, and ``schedule_end``
    behind the last epoch, into ``sched_ring`` (allocated beside the training log under ``log_capacity``; ``schedule_log()`` reads
    it).  All of it is state in device words, so a captured iteration anneals and stops at every replay.  Accumulates behind a
    closed gate still run and are discarded - the launch sequence is static -, and the training log's diagnostics columns still sum
    their rows.  With ``total_iterations`` None and ``kl_stop`` 0 the loop is what it always was."""

    def __init__(self, env, policy, fit, n_steps, gamma=0.99, lam=0.95, clip=0.2, ent_coef=0.01, epochs=4, minibatches=4, substeps=1,
                 normalize_advantages=False, obs_stats=None, std_min=1e-6, shuffle=False, seed=0, cliprange_vf=None, log_capacity=0,
                 normalize_rewards=False, reward_clip=10.0, reward_eps=1e-8, total_iterations=None, lr_end=None, clip_end=None,
                 cliprange_vf_end=None, ent_coef_end=None, kl_stop=0.0):
        (self.n_steps, self.gamma, self.lam, self.clip, self.ent_coef, self.epochs, self.minibatches,
         self.substeps) = check_pg_loop(n_steps, gamma, lam, clip, ent_coef, epochs, minibatches, substeps)
        self.shuffle, seed, self.cliprange_vf = check_pg_shuffle(shuffle, seed, cliprange_vf, self.n_steps, self.minibatches)
        self.log_capacity = _check_int("log_capacity", log_capacity, 0, 2 ** 31 - 1, "in 0 .. 2^31 - 1")
        self.normalize_advantages, self.obs_stats, self.std_min = bool(normalize_advantages), obs_stats, float(std_min)
        if not np.isfinite(self.std_min) or not (self.std_min > 0.0):
            raise ValueError("std_min must be finite and positive")
        self.grad_norms = None
        self._clipped = False
        self.normalize_rewards, self.update_reward_stats = bool(normalize_rewards), True
        _, _, _, _, self.reward_eps, self.reward_clip = check_reward_norm(self.n_steps, 1, 1, self.gamma, reward_eps, reward_clip)
        self.scheduled = total_iterations is not None or kl_stop != 0
        schedule = None
        if self.scheduled:
            ends = lambda a, b: (a, a if b is None else b)      # noqa: E731
            cv = 1.0 if self.cliprange_vf is None else self.cliprange_vf          # (never read without old values)
            if self.cliprange_vf is None and cliprange_vf_end is not None:
                raise ValueError("cliprange_vf_end needs cliprange_vf")
            schedule = check_pg_schedule(0 if total_iterations is None else total_iterations, ends(fit.lr, lr_end), ends(self.clip, clip_end),
                                         ends(cv, cliprange_vf_end), ends(self.ent_coef, ent_coef_end), kl_stop)
        elif any(x is not None for x in (lr_end, clip_end, cliprange_vf_end, ent_coef_end)):
            raise ValueError("lr_end, clip_end, cliprange_vf_end and ent_coef_end need total_iterations")
        self.kl_stop = schedule[5] if schedule else 0.0
        prop = getattr(env, "propagator", env)
        if not (prop.cfg.flags & _lib.FLAG_AUTO_RESET):
            raise ValueError("the env must be created with FLAG_AUTO_RESET: episodes restart inside the rollout")
        if policy.spec.value_hidden is None:
            raise ValueError("the policy has no value network")
        if fit.policy is not policy:
            raise ValueError("the fit is attached to another policy")
        if policy.device != prop.device:
            raise ValueError("the policy lives on device %d, the propagator on device %d" % (policy.device, prop.device))
        self.prop, self.policy, self.fit = prop, policy, fit
        T, n = self.n_steps, prop.n_envs
        self.n_envs = n
        sizes = {"obs": 8 * (T + 1) * 5 * n, "reward": 8 * T * n, "reason": T * n, "action": 4 * T * n, "logp": 4 * T * n,
                 "value": 4 * T * n, "last_value": 4 * n, "adv": 4 * T * n, "ret": 8 * T * n, "log": 64 * self.epochs * T,
                 "grad_norm_log": 16 * self.epochs * self.minibatches}
        if self.shuffle:
            check_pg_shuffle(True, seed, cliprange_vf, T, self.minibatches, n)          # (the gather's bound on n_steps * n_envs)
            M = (T // self.minibatches) * n
            sizes.update(shuffle_state=16, mb_obs=8 * 5 * M, mb_action=4 * M, mb_adv=4 * M, mb_logp=4 * M, mb_ret=8 * M, mb_value=4 * M)
            if self.normalize_advantages:
                sizes.update(adv_work=adv_normalize_work_bytes(n))
        elif self.normalize_advantages:
            sizes.update(adv_norm=4 * T * n, adv_work=adv_normalize_work_bytes(n))
        if self.log_capacity:
            check_pg_episodes(T, n, n, self.log_capacity)
            sizes.update(ep_return=8 * n, ep_len=4 * n, ep_work=pg_episodes_work_bytes(n), log_ring=8 * PG_LOG_COLS * self.log_capacity,
                         log_gen=8 * self.log_capacity, log_counter=8)
            if self.scheduled:
                sizes.update(sched_ring=8 * len(SCHED_LOG_COLUMNS) * self.log_capacity)
        if self.normalize_rewards:
            check_reward_norm(T, n, n, self.gamma, self.reward_eps, self.reward_clip)
            sizes.update(reward_norm=8 * T * n, ret_run=8 * n, reward_state=8 * REWARD_NORM_STATE_WORDS, reward_work=reward_norm_work_bytes(n))
        if obs_stats is not None:
            if obs_stats.n_envs < n or obs_stats.device != prop.device:
                raise ValueError("obs_stats: a statistics object of at least %d envs on device %d" % (n, prop.device))
            policy.set_obs_stats(obs_stats)                # (the rollouts of collect() feed it from now on)
        self._buf = {k: _hip.DeviceBuffer(b, prop.device) for k, b in sizes.items()}
        b, stream = self._buf, prop.stream_ptr()
        fills = [("obs", 0), ("action", 0), ("adv", 0), ("reason", 0)]         # (buffer, the byte it starts filled with)
        if self.log_capacity:              # every slot "never written" (all ones), everything else zero: fresh envs, iteration 0
            fills += [("ep_return", 0), ("ep_len", 0), ("ep_work", 0), ("log_ring", 0), ("log_counter", 0), ("log_gen", 0xFF)]
            fills += [("sched_ring", 0xFF)] if self.scheduled else []
        if self.normalize_rewards:         # a fresh state, fresh envs
            fills += [("reward_norm", 0), ("ret_run", 0), ("reward_state", 0), ("reward_work", 0)]
        # Whatever a first launch would allocate, here: the fit's scratch of block gradients for n samples, by an accumulate of zeros in
        # which no sample is alive - it adds +0.0 to every accumulator and nothing to the count.
        with _hip.device_guard(prop.device):
            for k, byte in fills:
                _hip.check(_hip.runtime().hipMemsetAsync(C.c_void_p(b[k].ptr), byte, sizes[k], C.c_void_p(stream)), "hipMemsetAsync")
            fit.accumulate_pg(b["obs"].ptr, b["action"].ptr, b["adv"].ptr, None, self.clip, 0.0, None, b["reason"].ptr, n=n, stride=n,
                              stream=stream)
        if self.shuffle:
            self.set_shuffle_state(seed, 0)
        if schedule:                       # (behind the accumulate of zeros above, which is an unscheduled launch like any before)
            fit.set_schedule(*schedule)

    # ------------------------------------------------------------------ host reads and writes of the device state
    @staticmethod
    def _need(flag, what):
        if not flag:
            raise ValueError("the loop was created without " + what)

    def _log_copy(self, pairs, upload):
        """Every (host array, buffer name) of ``pairs`` from the device, or with ``upload`` to it, behind a wait for the env"""
        self.prop.sync()
        with _hip.device_guard(self.prop.device):
            for host, name in pairs:
                h, d = C.c_void_p(host.ctypes.data), C.c_void_p(self._buf[name].ptr)
                if upload:
                    _hip.check(_hip.runtime().hipMemcpy(d, h, host.nbytes, _hip.hipMemcpyHostToDevice), "hipMemcpy")
                else:
                    _hip.check(_hip.runtime().hipMemcpy(h, d, host.nbytes, _hip.hipMemcpyDeviceToHost), "hipMemcpy")

    def schedule_log(self):
        """-> float64 (k, 8): the rows of ``SCHED_LOG_COLUMNS`` the schedule's ring holds, oldest first - one per ``update()``, the
        last ``log_capacity`` of them.  Synchronises."""
        self._need(self.scheduled and self.log_capacity, "a schedule or without log_capacity")
        rows = np.empty((self.log_capacity, len(SCHED_LOG_COLUMNS)), np.float64)
        self._log_copy(((rows, "sched_ring"),), False)
        return sched_log_table_ref(rows)

    def shuffle_state(self):
        """-> (seed, epoch), the two device words of the permutation (``shuffle=True`` only); epoch is the number of epochs run
        since ``set_shuffle_state``.  For checkpoints; synchronises."""
        self._need(self.shuffle, "shuffle")
        words = np.empty(2, np.uint64)
        self._log_copy(((words, "shuffle_state"),), False)
        return tuple(int(w) for w in words)

    def set_shuffle_state(self, seed, epoch=0):
        """The two words back: with them, and the fit's state, an update resumes bit for bit.  Synchronises."""
        seed = check_pg_shuffle(True, seed)[1]
        epoch = _check_int("epoch", epoch, 0, 2 ** 64 - 1, "in 0 .. 2^64 - 1")
        self._need(self.shuffle, "shuffle")
        self._log_copy(((np.array([seed, epoch], np.uint64), "shuffle_state"),), True)

    def training_log(self):
        """-> (iterations uint64 (k,), rows float64 (k, 26)): the slots of the ring that have been written, oldest first - one row of
        ``PG_LOG_COLUMNS`` per ``collect()`` + ``update()``, the last ``log_capacity`` of them.  Synchronises."""
        self._need(self.log_capacity, "log_capacity")
        gen, rows = np.empty(self.log_capacity, np.uint64), np.empty((self.log_capacity, PG_LOG_COLS), np.float64)
        self._log_copy(((gen, "log_gen"), (rows, "log_ring")), False)
        return pg_log_table_ref(gen, rows)

    def episode_state(self):
        """-> (ep_return float64 (n,), ep_len int32 (n,), counter): the return and the length of every env's running episode and the
        number of the iteration being written.  For checkpoints; synchronises."""
        self._need(self.log_capacity, "log_capacity")
        R, L, c = np.empty(self.n_envs, np.float64), np.empty(self.n_envs, np.int32), np.empty(1, np.uint64)
        self._log_copy(((R, "ep_return"), (L, "ep_len"), (c, "log_counter")), False)
        return R, L, int(c[0])

    def set_episode_state(self, ep_return, ep_len, counter=0):
        """The three back: with them - and the env's own state - the log goes on as if it had not been interrupted (the ring's rows
        are not part of it).  Synchronises."""
        self._need(self.log_capacity, "log_capacity")
        R, L = np.ascontiguousarray(ep_return, np.float64).reshape(-1), np.ascontiguousarray(ep_len, np.int32).reshape(-1)
        if R.size != self.n_envs or L.size != self.n_envs:
            raise ValueError("ep_return and ep_len: one value per env (%d)" % self.n_envs)
        counter = _check_int("counter", counter, 0, 2 ** 64 - 1, "in 0 .. 2^64 - 1")
        self._log_copy(((R, "ep_return"), (L, "ep_len"), (np.array([counter], np.uint64), "log_counter")), True)

    def reward_norm_state(self):
        """-> (state uint64 (8,), ret_run float64 (n,)): the words of the reward statistics as the device holds them
        (``policy_ref.REWARD_NORM_STATE_FIELDS``) and every env's running discounted return (``normalize_rewards=True`` only).  For
        checkpoints; synchronises."""
        self._need(self.normalize_rewards, "normalize_rewards")
        words, R = np.empty(REWARD_NORM_STATE_WORDS, np.uint64), np.empty(self.n_envs, np.float64)
        self._log_copy(((words, "reward_state"), (R, "ret_run")), False)
        return words, R

    def set_reward_norm_state(self, state, ret_run):
        """The two back: with them - and the env's own state - the scaling goes on as if it had not been interrupted.
        Synchronises."""
        self._need(self.normalize_rewards, "normalize_rewards")
        words = reward_norm_state_words(np.ascontiguousarray(state))
        R = np.ascontiguousarray(ret_run, np.float64).reshape(-1)
        if R.size != self.n_envs:
            raise ValueError("ret_run: one value per env (%d)" % self.n_envs)
        self._log_copy(((words, "reward_state"), (R, "ret_run")), True)

    def reward_scale(self):
        """-> float: what ``collect()`` divides the rewards by as the statistics stand - the running standard deviation of the
        discounted return, 1.0 before the first rollout.  A value of the value network times this is in the reward's own unit.
        Synchronises."""
        return float(reward_norm_divisor(self.reward_norm_state()[0]))

    def close(self):
        if getattr(self, "_buf", None):
            self.prop.sync()
            for b in self._buf.values():
                b.free()
            self._buf = None
            if self.scheduled and self.fit._p:         # (a fit closed before the loop has no schedule left to clear)
                self.fit.clear_schedule()
            if self.obs_stats is not None:
                self.policy.set_obs_stats(None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def buffers(self):
        """-> the device pointers of the loop's buffers by name: ``obs`` f64[n_steps + 1][5][n] (row t: what the action of step t
        was chosen from), ``reward`` f64, ``reason`` u8, ``action`` i32, ``logp`` f32, ``value`` f32, ``adv`` f32, ``ret`` f64
        [n_steps][n], ``last_value`` f32[n], ``log`` f64[epochs][n_steps][8] (the two diagnostics rows of every accumulate),
        ``grad_norm_log`` f64[epochs * minibatches][2] (written under ``fit.max_grad_norm`` only) and, with
        ``normalize_advantages``, ``adv_norm`` f32[n_steps][n] - every minibatch's rows normalised on their own, what ``update()``
        reads - and ``adv_work``, the scratch of ``bsk_adv_normalize``.  With ``shuffle``: ``shuffle_state`` u64[2] = {seed, epoch}
        and the gathered minibatch of M = (n_steps // minibatches) * n samples, ``mb_obs`` f64[5][M], ``mb_action`` i32,
        ``mb_adv`` f32 (normalised in place under ``normalize_advantages``; there is then no ``adv_norm``), ``mb_logp`` f32,
        ``mb_ret`` f64 and ``mb_value`` f32 [M] (written under ``cliprange_vf`` only).  With ``log_capacity``: ``ep_return`` f64[n]
        and ``ep_len`` i32[n] (every env's running episode), ``ep_work`` (the scratch of ``bsk_pg_episodes``), ``log_ring``
        f64[log_capacity][26], ``log_gen`` u64[log_capacity] (the iteration each slot holds; all ones: never written) and
        ``log_counter`` u64 (the iteration being written) and, with a schedule, ``sched_ring`` f64[log_capacity][8] (rows of
        ``SCHED_LOG_COLUMNS``; a NaN iteration: never written).  With ``normalize_rewards``: ``reward_norm`` f64[n_steps][n] (the scaled
        and clipped rewards, what ``bsk_gae`` reads; ``reward`` keeps the raw ones), ``ret_run`` f64[n] (every env's running
        discounted return), ``reward_state`` u64[8] (the statistics) and ``reward_work`` (the scratch of ``bsk_reward_norm``)"""
        return {k: b.ptr for k, b in self._buf.items()}

    def collect(self):
        """The handle's observation into row 0, a sampled rollout of ``n_steps`` that fills the histories (observations from row 1),
        the value of the observation the handle holds afterwards, and ``bsk_gae``: all enqueued on the env's stream.  In front of
        all of it, with ``obs_stats``: the statistics so far into the policy's input normalisation; between the value and
        ``bsk_gae``, with ``normalize_rewards``: ``reward`` scaled into ``reward_norm``, which ``bsk_gae`` then reads, the
        statistics updated first unless ``update_reward_stats`` is False at this moment; behind all of it, with
        ``normalize_advantages`` and without ``shuffle``: every minibatch's rows of ``adv`` normalised into ``adv_norm`` (with
        ``shuffle`` the minibatches do not exist yet: ``update()`` normalises each behind its gather)."""
        prop, b, T, n = self.prop, self._buf, self.n_steps, self.n_envs
        stream = prop.stream_ptr()
        if self.obs_stats is not None:
            self.fit.apply_obs_norm(self.obs_stats, self.std_min, stream)
        views = prop.device_views()
        obs, stride = views["obs"].__cuda_array_interface__["data"][0], views["stride"]
        with _hip.device_guard(prop.device):
            _hip.memcpy2d_async(b["obs"].ptr, 8 * n, obs, 8 * stride, 8 * n, 5, _hip.hipMemcpyDeviceToDevice, stream)
            self.policy.rollout_device(prop, T, self.substeps, "sample", b["obs"].ptr + 8 * 5 * n, b["reward"].ptr, b["reason"].ptr,
                                       b["action"].ptr, b["logp"].ptr, b["value"].ptr)
            self.policy.value_enqueue(obs, stride, n, b["last_value"].ptr, stream)
            reward = b["reward"].ptr
            if self.normalize_rewards:
                reward = b["reward_norm"].ptr
                reward_normalize(b["reward"].ptr, b["reason"].ptr, T, n, b["reward_state"].ptr, reward, b["ret_run"].ptr, b["reward_work"].ptr,
                                 self.gamma, self.reward_eps, self.reward_clip, self.update_reward_stats, stream=stream)
            gae(reward, b["reason"].ptr, b["value"].ptr, b["last_value"].ptr, T, n, b["adv"].ptr, b["ret"].ptr, self.gamma,
                self.lam, stream=stream)
            if self.normalize_advantages and not self.shuffle:
                rows = T // self.minibatches
                for g in range(self.minibatches):
                    normalize_advantages(b["adv"].ptr + 4 * n * rows * g, rows, n, b["adv_norm"].ptr + 4 * n * rows * g,
                                         work=b["adv_work"].ptr, stream=stream)
            if self.log_capacity:
                pg_episodes(b["reward"].ptr, b["reason"].ptr, T, n, b["ep_return"].ptr, b["ep_len"].ptr, b["ep_work"].ptr, b["log_ring"].ptr,
                            self.log_capacity, b["log_counter"].ptr, b["action"].ptr, b["value"].ptr, b["ret"].ptr, stream=stream)

    def update(self):
        """``epochs`` passes of ``minibatches`` groups of consecutive time rows: per row one ``accumulate_pg`` of the n envs and its
        two diagnostics rows into the log, device to device (a row is one accumulate's: ``iterate`` adds a group's on the host,
        behind its wait); per group one ``fit.step()`` and, under ``fit.max_grad_norm``, its {norm, scale} row into a log of its
        own.  With ``shuffle`` a group is a gathered minibatch and a row a chunk of n of its samples (``epoch``)."""
        self._clipped = self.fit.max_grad_norm > 0.0
        if self.scheduled:
            self.fit.schedule_begin(self.prop.stream_ptr())
        for e in range(self.epochs):
            self.epoch(e)
        if self.scheduled:
            ring = self._buf["sched_ring"].ptr if self.log_capacity else None
            self.fit.schedule_end(ring, self.log_capacity, self.prop.stream_ptr())
        if self.log_capacity:
            b, stream = self._buf, self.prop.stream_ptr()
            with _hip.device_guard(self.prop.device):
                pg_log_update(b["log"].ptr, self.epochs * self.n_steps, b["log_ring"].ptr, self.log_capacity, b["log_counter"].ptr,
                              b["grad_norm_log"].ptr if self._clipped else None, self.epochs * self.minibatches, stream=stream)
                pg_log_advance(b["log_gen"].ptr, self.log_capacity, b["log_counter"].ptr, stream)

    def epoch(self, e=0):
        """One pass of ``update()`` over the minibatches, enqueued on the env's stream: its diagnostics rows go to the log's rows of
        pass ``e``.  Without ``shuffle``: the groups of consecutive time rows, one accumulate per row.  With it, per minibatch g:
        one ``pg_gather`` of the M samples perm(g M) .. perm(g M + M - 1) into ``mb_*``, under ``normalize_advantages`` their
        normalisation in place, then one accumulate per chunk of n of them; and behind the pass ``pg_shuffle_advance``, so that
        the next pass - or the next replay of this one from a graph - draws another permutation.  Under ``cliprange_vf`` the
        accumulates are ``accumulate_ppo`` against the recorded values."""
        prop, b, n, T, fit = self.prop, self._buf, self.n_envs, self.n_steps, self.fit
        clipped, cv = fit.max_grad_norm > 0.0, self.cliprange_vf
        gn_row = fit.grad_norm_ptr() if clipped else None
        stream, rows = prop.stream_ptr(), T // self.minibatches
        pg_row, fit_row = fit.pg_stats_ptr(), fit.stats_ptr()
        M, log = rows * n, b["log"].ptr
        # where a row's samples come from: obs, actions, advantages, old log-probabilities, returns and old values, and the row stride
        if self.shuffle:
            names, stride = ("mb_obs", "mb_action", "mb_adv", "mb_logp", "mb_ret", "mb_value"), M
        else:
            names, stride = ("obs", "action", "adv_norm" if self.normalize_advantages else "adv", "logp", "ret", "value"), n
        obs, act, adv, logp, ret, val = (b[k].ptr for k in names)
        with _hip.device_guard(prop.device):
            slot = int(e) * T
            for g in range(self.minibatches):
                if self.shuffle:
                    old = (b["value"].ptr, val) if cv is not None else (None, None)
                    pg_gather(b["shuffle_state"].ptr, T, n, g * M, M, b["obs"].ptr, b["action"].ptr, b["adv"].ptr, b["logp"].ptr,
                              b["ret"].ptr, old[0], obs, act, adv, logp, ret, old[1], stream=stream)
                    if self.normalize_advantages:
                        normalize_advantages(adv, rows, n, work=b["adv_work"].ptr, stream=stream)
                for c in range(rows):
                    at = n * (c if self.shuffle else g * rows + c)         # the row's first sample
                    o = obs + 8 * (at if self.shuffle else 5 * at)         # (a gathered minibatch is [5][M], the history [T][5][n])
                    if cv is None:
                        fit.accumulate_pg(o, act + 4 * at, adv + 4 * at, logp + 4 * at, self.clip, self.ent_coef, ret + 8 * at, None, n=n,
                                          stride=stride, stream=stream)
                    else:
                        fit.accumulate_ppo(o, act + 4 * at, adv + 4 * at, logp + 4 * at, self.clip, self.ent_coef, ret + 8 * at,
                                           val + 4 * at, cv, None, n=n, stride=stride, stream=stream)
                    _copy_row(log + 64 * slot, pg_row, 32, stream)
                    _copy_row(log + 64 * slot + 32, fit_row, 32, stream)
                    slot += 1
                if self.kl_stop > 0.0:     # (over this minibatch's rows of the log, which the copies above have just written)
                    fit.kl_gate(log + 64 * (slot - rows), rows, stream)
                fit.step(stream)
                if clipped:
                    _copy_row(b["grad_norm_log"].ptr + 16 * (slot // rows - 1), gn_row, 16, stream)
            if self.shuffle:
                pg_shuffle_advance(b["shuffle_state"].ptr, stream)

    def iterate(self):
        """``collect()`` then ``update()`` -> float64 (epochs * minibatches, 8): per minibatch ``PG_STATS_COLUMNS`` then
        ``FIT_STATS_COLUMNS``, each the sum over the minibatch's rows in their order, formed after the one wait at the end.
        ``grad_norms`` is afterwards the {norm, scale} row of every step, float64 (epochs * minibatches, 2), or None without
        ``fit.max_grad_norm``."""
        out = np.empty((self.epochs * self.minibatches, self.n_steps // self.minibatches, 8), np.float64)
        self.collect()
        self.update()
        norms = np.empty((self.epochs * self.minibatches, 2), np.float64) if self._clipped else None
        with _hip.device_guard(self.prop.device):
            if norms is not None:
                _hip.check(_hip.runtime().hipMemcpyAsync(C.c_void_p(norms.ctypes.data), C.c_void_p(self._buf["grad_norm_log"].ptr), norms.nbytes,
                                                         _hip.hipMemcpyDeviceToHost, C.c_void_p(self.prop.stream_ptr())), "hipMemcpyAsync")
            _hip.check(_hip.runtime().hipMemcpyAsync(C.c_void_p(out.ctypes.data), C.c_void_p(self._buf["log"].ptr), out.nbytes,
                                                     _hip.hipMemcpyDeviceToHost, C.c_void_p(self.prop.stream_ptr())), "hipMemcpyAsync")
        self.prop.sync()
        self.grad_norms = norms
        log = np.zeros((out.shape[0], 8), np.float64)
        for k in range(out.shape[1]):
            log = log + out[:, k]
        return log
