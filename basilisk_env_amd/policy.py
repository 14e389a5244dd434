"""A small MLP policy evaluated on the GPU by the library itself, and closed-loop rollouts built from it: the ctypes bindings.

``DevicePolicy`` holds one or two multilayer perceptrons over the five observation rows (``bsk_policy_*``, include/bskgpu.h): the
action network (5 -> hidden... -> 3 logits) and an optional value network (5 -> hidden... -> 1).  ``act`` is ONE launch that reads
the observation rows where the step kernel leaves them and writes int32 actions ``step_device`` reads in place (plus, when asked,
log-probability, value and logits); ``rollout`` closes the loop on the device for whole episodes.  Both are enqueue-only and can be
captured into a HIP graph.  An extra beside the reference surface: the reference's agent runs its network in
stable-baselines, outside the env.

``PolicyPopulation`` holds P parameter sets of one spec (``bsk_population_*``): member m drives envs [m * E, (m + 1) * E) of one
propagator, one launch per env step serves all members, and the per-member fitness of a rollout is formed on the device.
``DeviceEvolutionStrategy`` (``bsk_es_*``) keeps theta on the device and asks, ranks and updates there, its noise regenerated from
a counter instead of stored.  ``ObsStats`` (``bsk_obs_stats_*``) keeps running sums of the observation rows on the device: attached to
a population or a policy it is fed by their rollouts, and ``DeviceEvolutionStrategy.apply_obs_norm`` turns it into theta's in_scale
and in_shift.  ``PolicyFit`` (``bsk_fit_*``; its binding lives in ``policy_fit`` and is re-exported here) is the gradient side: a
supervised fit of a ``DevicePolicy`` to labels that are already on the device, such as a planner's - and, with ``gae``
(``bsk_gae``), ``PolicyFit.accumulate_pg`` and the loop ``PolicyGradient`` over them, training by the reward itself (PPO / A2C),
conditioned as PPO2 conditions it by ``normalize_advantages`` (``bsk_adv_normalize``), ``PolicyFit.max_grad_norm`` and
``PolicyFit.apply_obs_norm``, fed shuffled minibatches by ``pg_gather`` (``bsk_pg_gather``; ``pg_perm_ref``) and given PPO2's
clipped value loss by ``PolicyFit.accumulate_ppo`` (``fit_value_delta_ref``); ``PolicyGradient(log_capacity=)`` keeps a per-iteration
training log on the device (``pg_episodes`` / ``pg_log_update`` / ``pg_log_advance``; ``pg_episodes_ref``, ``PG_LOG_COLUMNS``) and
``PolicyGradient(normalize_rewards=True)`` divides the rewards by the running deviation of the discounted return
(``reward_normalize``, ``bsk_reward_norm``; ``reward_norm_ref``); ``PolicyFit.set_schedule`` keeps lr, clip, clip_vf and ent_coef
in device words the fit's kernels read, annealed per iteration, with a KL stop per update (``bsk_fit_set_schedule``, ...;
``pg_schedule_ref``, ``fit_kl_gate_ref``) - ``PolicyGradient(total_iterations=, lr_end=, clip_end=, kl_stop=)``.

They are handles of the library and share what such a handle needs (``policy_base._DeviceObject``: create, close, the closed-handle
refusal, ``sync``); the policy and the population are also both parameter stores that act (``_ParamStore``: the draw counter, the
output buffers and views of ``act``, rollouts with host results) - as ``ParamStore`` is behind the two in csrc/bsk_capi_policy.hip;
``bsk_es_*`` is csrc/bsk_capi_es.hip.

What needs no device lives beside this module and is re-exported here under the names it always had: the argument rules and the
layout of the parameter block in ``policy_spec`` (``check_spec``, ``pack_params``, ...), and in ``policy_ref`` the numpy
restatements the kernels are held to bit for bit (``mlp_ref`` / ``act_ref``: every layer output one k-ordered chain of f32 fused
multiply-adds from the bias; ``population_fitness_ref``; ``es_noise_ref`` / ``es_ask_ref`` / ``es_tell_ref`` /
``es_tell_adam_ref`` / ``es_ask_sigma_ref`` / ``es_tell_pgpe_ref`` / ``es_log_row_ref`` / ``es_best_ref`` / ``es_center_ref`` / ``es_validate_ref``;
``population_outcomes_ref`` / ``es_outcome_row_ref``; ``obs_stats_accumulate_ref`` / ``obs_stats_totals_ref`` / ``obs_norm_ref``) with ``EvolutionStrategy``, the host-side loop the device one was modelled on.
"""
import ctypes as C

import numpy as np

from . import _hip, _lib
from ._lib import check
from .policy_base import _DeviceObject, _host_block  # noqa: F401
from .policy_fit import PolicyFit, PolicyGradient, gae, normalize_advantages, pg_gather, pg_shuffle_advance  # noqa: F401
from .policy_fit import pg_episodes, pg_log_advance, pg_log_update  # noqa: F401
from .policy_fit import reward_normalize  # noqa: F401
from .policy_ref import (REWARD_NORM_STATE_FIELDS, REWARD_NORM_STATE_WORDS, check_reward_norm, reward_norm_divisor,  # noqa: F401
                         reward_norm_ref, reward_norm_state_words, reward_norm_walk_ref, reward_norm_work_bytes)
from .policy_ref import (SCHED_LOG_COLUMNS, SCHED_STATE_FIELDS, SCHED_WORDS, check_pg_schedule, fit_kl_gate_ref,  # noqa: F401
                         pg_schedule_ref, sched_log_table_ref, sched_words_ref)
from .policy_ref import (PG_LOG_COLS, PG_LOG_COLUMNS, check_pg_episodes, check_pg_log, pg_episodes_ref, pg_episodes_walk_ref,  # noqa: F401
                         pg_episodes_work_bytes, pg_log_table_ref, pg_log_update_ref)
from .policy_ref import (VCLIP_STATS_COLUMNS, check_pg_gather, check_pg_shuffle, fit_value_delta_ref, pg_gather_ref,  # noqa: F401
                         pg_perm_keys_ref, pg_perm_ref, pg_shuffle_keys_ref)
from .policy_ref import (FIT_BLOCK, FIT_STATS_COLUMNS, check_fit, check_fit_batch, fit_accumulate_ref, fit_backward_ref,  # noqa: F401
                         fit_dlogits32_ref, fit_dlogits_ref, fit_loss_ref, fit_stats_ref, fit_step_ref)
from .policy_ref import (PG_STATS_COLUMNS, check_gae, check_pg, check_pg_loop, fit_pg_dlogits32_ref, fit_pg_dlogits_ref,  # noqa: F401
                         fit_pg_loss_ref, fit_pg_stats_ref, fit_pg_terms_ref, gae_ref, pg_clip_edges)
from .policy_ref import (adv_normalize_ref, adv_normalize_work_bytes, check_adv_normalize, check_max_grad_norm,  # noqa: F401
                         fit_grad_norm_ref)
from .policy_ref import (ES_LOG_COLUMNS, ES_LOG_EMPTY, ES_VAL_COLUMNS, ES_VAL_MAX_MEMBERS, EvolutionStrategy, _es_pair_sum,  # noqa: F401
                         _es_pair_sums, _series_log, act_ref,
                         centred_ranks, check_adam, check_log, check_validation,
                         es_ask_ref, es_ask_sigma_ref, es_best_ref, es_center_ref, es_champion_empty, es_inverse_normal_ref, es_log_order_ref,
                         es_log_row_ref, es_log_slot_ref, es_log_table_ref, es_noise_ref, es_outcome_row_ref, es_outcome_table_ref,
                         es_tell_adam_ref, es_tell_pgpe_ref,
                         es_tell_ref, es_uniform_ref, es_validate_ref, es_validation_state, es_validation_table_ref, fma32,
                         mlp_ref, obs_moments_ref, obs_norm_ref, obs_stats_accumulate_ref, obs_stats_totals_ref,
                         obs_stats_zero_state, outcome_table_ref, philox4x32_10, population_fitness_ref, population_outcomes_ref, sample_uniform,
                         shared_slot_ref, softmax_ref)
from .policy_spec import (ACTIVATIONS, MAX_HIDDEN_LAYERS, MODES, OUTCOME_COLS, OUTCOME_COLUMNS, POLICY_GREEDY, POLICY_RELU,  # noqa: F401
                          POLICY_SAMPLE, POLICY_TANH, BskPolicySpec, Spec, _as_spec, c_spec, check_outcome_log,
                          check_sigma_adaptation, check_spec, layer_shapes,
                          n_params, pack_params,
                          torch_layers, unpack_params)


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


class _ParamStore(_DeviceObject):
    """What the policy and the population share beyond the handle: the draw counter of sample mode, the output buffers ``act``
    writes and the views it returns, and rollouts whose results come back to the host."""
    _out_n = 0

    def set_rng(self, seed, draw=0):
        check(self._c("set_rng")(self._handle(), int(seed), int(draw)))

    def get_rng(self):
        """-> (seed, draw); synchronises."""
        s, d = C.c_uint64(), C.c_uint64()
        check(self._c("get_rng")(self._handle(), C.byref(s), C.byref(d)))
        return s.value, d.value

    def _buffers(self, n):
        if self._out is None or self._out_n < n:
            if self._out:
                self.sync()
                for b in self._out.values():
                    b.free()
            self._out = {"action": _hip.DeviceBuffer(4 * n, self.device), "logp": _hip.DeviceBuffer(4 * n, self.device),
                         "value": _hip.DeviceBuffer(4 * n, self.device), "logits": _hip.DeviceBuffer(12 * n, self.device)}
            self._out_n = n
        return self._out

    def _outputs(self, n, want):
        """-> the output buffers for n spacecraft, and the four output arguments of an act launch: ``action`` always, of ``logp``,
        ``value`` and ``logits`` those that ``want`` names"""
        out = self._buffers(n)
        return out, [C.c_void_p(out["action"].ptr)] + [C.c_void_p(out[k].ptr) if k in want else None for k in ("logp", "value", "logits")]

    def _act(self, source, mode, want, env_base, stream, launch):
        """``act`` around ``launch(ptr, stride, n, want, env_base, stream)`` -> the output buffers: the argument rules before it,
        the resolved source into it, the dict of device views after it."""
        from .simulators.dynamics.propagator import _DevArray
        if mode not in MODES:
            raise ValueError("mode must be 'greedy' or 'sample'")
        want = tuple(want)
        for w in want:
            if w not in ("logp", "value", "logits"):
                raise ValueError("want: 'logp', 'value' and / or 'logits', got %r" % (w,))
        if "value" in want and self.spec.value_hidden is None:
            raise ValueError("want 'value': the %s has no value network" % self._what)
        ptr, stride, n, stream, env_base, owner = _observation_source(self, source, env_base, stream)
        out = launch(ptr, stride, n, want, env_base, stream)
        kw = {"owner": owner, "device": self.device, "stream": stream}
        res = {"action": _DevArray(out["action"].ptr, (n,), "<i4", **kw)}
        for name in want:
            res[name] = _DevArray(out[name].ptr, (3, n) if name == "logits" else (n,), "<f4", **kw)
        return res

    def _host_rollout(self, prop, host, launch):
        """Fills the numpy arrays of ``host`` from a rollout: one device buffer per array, ``launch({name: pointer})`` to enqueue the
        rollout that writes them, the copies back on the propagator's stream, one ``prop.sync()``.  -> ``host``"""
        bufs = {k: _hip.DeviceBuffer(a.nbytes, self.device) for k, a in host.items()}
        try:
            launch({k: b.ptr for k, b in bufs.items()})
            stream = C.c_void_p(prop.stream_ptr())
            for k, dst in host.items():
                _hip.check(_hip.runtime().hipMemcpyAsync(C.c_void_p(dst.ctypes.data), C.c_void_p(bufs[k].ptr), dst.nbytes,
                                                         _hip.hipMemcpyDeviceToHost, stream), "hipMemcpyAsync")
            prop.sync()
        finally:
            for b in bufs.values():
                b.free()
        return host


    def set_obs_stats(self, stats):
        """Attaches an ``ObsStats`` (None detaches): from then on the rollouts accumulate, in front of every launch of the policy,
        the observation the action is chosen from - one more launch per env step - and join once behind the last step.  Under a
        population rollout that forms fitness only the episode that counts towards it is counted.  The object is kept alive, not
        owned: close it after detaching."""
        check(self._c("set_obs_stats")(self._handle(), None if stats is None else stats._handle()))
        self._stats = stats


class ObsStats(_DeviceObject):
    """Running sums, sums of squares and counts of the five observation rows for up to ``n_envs`` spacecraft, on the device
    (``bsk_obs_stats_*``): fed by ``accumulate`` or by the rollouts of what it is attached to (``set_obs_stats``), in a fixed
    order and without atomics, so that ``obs_stats_accumulate_ref`` / ``obs_stats_totals_ref`` repeat it bit for bit.  Not
    thread-safe, one stream at a time."""
    _kind, _what = "obs_stats", "observation statistics"

    def __init__(self, n_envs, device=0):
        self.n_envs = int(n_envs)
        self.waves = (self.n_envs + 63) // 64
        self._create(device, self.n_envs)

    def accumulate(self, obs, n=None, stride=None, alive=None, stream=0):
        """``obs``: a device array (5, n) float64 with contiguous rows (``__cuda_array_interface__``), or a raw pointer to
        f64[5][stride] with ``n`` (``stride`` defaults to n); ``alive``: a raw device pointer to n bytes, an array of them, or None
        (every spacecraft counts).  Two launches on ``stream``: no copy, no synchronisation, capturable."""
        cai = getattr(obs, "__cuda_array_interface__", None)
        if cai is not None:
            shape, strides = tuple(cai["shape"]), cai.get("strides")
            if cai["typestr"] != "<f8" or len(shape) != 2 or shape[0] != 5 or shape[1] < 1:
                raise ValueError("observations: a float64 device array of shape (5, n), got %r %r" % (cai["typestr"], shape))
            strides = (shape[1] * 8, 8) if strides is None else tuple(strides)
            if strides[1] != 8 or strides[0] % 8 or strides[0] < shape[1] * 8:
                raise ValueError("observations: rows must be contiguous and at least n elements apart")
            self._source, obs, n, stride = obs, int(cai["data"][0]), shape[1], strides[0] // 8
        elif n is None:
            raise ValueError("a raw observation pointer needs n")
        stride = int(n) if stride is None else int(stride)
        a = getattr(alive, "__cuda_array_interface__", None)
        if a is not None:
            if a["typestr"] not in ("|u1", "|b1") or int(np.prod(a["shape"])) != int(n):
                raise ValueError("alive: %d bytes, got %r %r" % (n, a["typestr"], a["shape"]))
            self._alive, alive = alive, int(a["data"][0])
        check(self._lib.bsk_obs_stats_accumulate(self._handle(), C.c_void_p(int(obs)) if obs else None, stride, int(n),
                                                 C.c_void_p(int(alive)) if alive else None, C.c_void_p(int(stream or 0))))

    def _get(self):
        n, mean, var = C.c_uint64(), np.empty(5, np.float64), np.empty(5, np.float64)
        check(self._lib.bsk_obs_stats_get(self._handle(), C.byref(n), mean.ctypes.data, var.ctypes.data))
        return n.value, mean, var

    @property
    def count(self):
        """The number of observations counted; synchronises."""
        return self._get()[0]

    @property
    def mean(self):
        """float64 (5,), zeros while nothing is counted; synchronises."""
        return self._get()[1]

    @property
    def var(self):
        """float64 (5,), E[x^2] - mean^2 clamped at zero (``obs_moments_ref``); synchronises."""
        return self._get()[2]

    @property
    def state(self):
        """(part float64 (W, 10), cnt uint64 (W,)), W = ceil(n_envs / 64): what a checkpoint keeps; synchronises."""
        part, cnt = np.empty((self.waves, 10), np.float64), np.empty(self.waves, np.uint64)
        check(self._lib.bsk_obs_stats_get_state(self._handle(), part.ctypes.data, cnt.ctypes.data))
        return part, cnt

    def set_state(self, part, cnt):
        """The partial rows back (``state``'s shapes); the totals are formed again.  Synchronises."""
        part = _host_block(part, 10, np.float64, rows=self.waves, what="partial sums")
        cnt = _host_block(cnt, self.waves, np.uint64, what="counts")
        check(self._lib.bsk_obs_stats_set_state(self._handle(), part.ctypes.data, cnt.ctypes.data))

    def reset(self, stream=0):
        """Everything back to zero: one memset on ``stream``."""
        check(self._lib.bsk_obs_stats_reset(self._handle(), C.c_void_p(int(stream or 0))))

    def totals_ptr(self):
        """-> (pointer to tot float64[10], pointer to the count uint64): DEVICE words, valid until ``close``, as fresh as the last
        join."""
        t, n = C.c_void_p(), C.c_void_p()
        check(self._lib.bsk_obs_stats_totals_device(self._handle(), C.byref(t), C.byref(n)))
        return t.value, n.value


class DevicePolicy(_ParamStore):
    """The policy on one GPU.  ``spec``: a ``Spec`` (``check_spec``); ``params``: its float32 parameter block (``pack_params``).
    Not thread-safe, and one stream at a time: the draw counter and the output buffers are single.  Output buffers are sized for
    the largest batch seen so far; a call that must grow them allocates, so make the first call of a size outside a graph capture."""
    _kind = _what = "policy"

    def __init__(self, spec, params, device=0):
        self.spec = _as_spec(spec)
        p = _host_block(params, n_params(self.spec))
        self._create(device, p.ctypes.data)

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

    def set_params(self, params):
        p = _host_block(params, n_params(self.spec))
        check(self._lib.bsk_policy_set_params(self._handle(), p.ctypes.data))

    # ------------------------------------------------------------------ evaluation
    def enqueue(self, obs_ptr, obs_stride, n, mode="greedy", want=(), env_base=0, stream=0):
        """``bsk_policy_act`` on raw arguments (what ``act`` resolves its source to, for loops that resolve it once): observations
        f64[5][obs_stride] at ``obs_ptr``.  -> the policy's output buffers by name (``_hip.DeviceBuffer``: ``action`` int32[n],
        ``logp`` / ``value`` f32[n], ``logits`` f32[3][n]); only ``action`` and the names in ``want`` are written."""
        if mode not in MODES:
            raise ValueError("mode must be 'greedy' or 'sample'")
        out, outputs = self._outputs(int(n), want)
        check(self._lib.bsk_policy_act(self._handle(), C.c_void_p(int(obs_ptr)), int(obs_stride), int(n), int(env_base), MODES[mode],
                                       *outputs, int(n), C.c_void_p(int(stream))))
        return out

    def value_enqueue(self, obs_ptr, obs_stride, n, out_ptr, stream=0):
        """``bsk_policy_value`` on raw arguments: the value network alone for observations f64[5][obs_stride] at ``obs_ptr``, one
        launch on ``stream`` that writes f32[n] at ``out_ptr`` - bit for bit what ``enqueue(..., want=("value",))`` leaves in
        ``value``.  No action network, no draw counter, no output buffer of the policy: it allocates nothing and is capturable from
        the first call (what the planners read at their leaves, ``planning.LookaheadPlanner(value_policy=...)``)."""
        check(self._lib.bsk_policy_value(self._handle(), C.c_void_p(int(obs_ptr)) if obs_ptr else None, int(obs_stride), int(n),
                                         C.c_void_p(int(out_ptr)) if out_ptr else None, C.c_void_p(int(stream or 0))))

    def act(self, source, mode="greedy", want=("logp", "value", "logits"), env_base=None, stream=None):
        """One launch: actions (and what ``want`` names) for every spacecraft of ``source`` - a ``BatchedPropagator`` (or an env
        with a ``propagator``): its own observation buffers, stream and env_base - or any device array of shape (5, n) float64 with
        contiguous rows (``__cuda_array_interface__``: a torch tensor, a propagator view), evaluated on ``stream`` (an integer
        hipStream_t, default the null stream).  Enqueue-only: no copy, no synchronisation.
        -> dict of device views (``__cuda_array_interface__`` / DLPack) valid until the next call: ``action`` int32 (n,) - whose
        pointer ``step_device`` takes as it is - and ``logp`` (n,), ``value`` (n,), ``logits`` (3, n) float32 where wanted."""
        return self._act(source, mode, want, env_base, stream,
                         lambda ptr, stride, n, want, env_base, stream: self.enqueue(ptr, stride, n, mode, want, env_base, stream))

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
        prop = getattr(prop, "propagator", prop)
        n, T = prop.n_envs, int(n_steps)
        names = [("obs", np.float64, (T, 5, n)), ("reward", np.float64, (T, n)), ("reason", np.uint8, (T, n)),
                 ("action", np.int32, (T, n)), ("logp", np.float32, (T, n))]
        if self.spec.value_hidden is not None:
            names.append(("value", np.float32, (T, n)))
        host = {k: np.empty(shape, dtype=dt) for k, dt, shape in names}
        return self._host_rollout(prop, host, lambda d: self.rollout_device(prop, T, substeps, mode,
                                                                            **{"d_%s_hist" % k: p for k, p in d.items()}))


class PolicyPopulation(_ParamStore):
    """``n_members`` parameter sets of one ``spec`` on one GPU.  With ``envs_per_member`` = E (a multiple of 64), spacecraft j is
    driven by member j // E: ONE policy launch per env step serves every member, and ``rollout_device`` / ``evaluate`` form the
    per-member fitness on the device (``population_fitness_ref`` restates it).  ``params``: float32 (P, n_params), one
    ``pack_params`` block per row, or None with ``n_members`` given (all-zero members).  Not thread-safe, one stream at a time,
    like ``DevicePolicy``."""
    _kind = _what = "population"

    def __init__(self, spec, params=None, device=0, n_members=None):
        self.spec = _as_spec(spec)
        self.n_params = n_params(self.spec)
        if params is None:
            if n_members is None:
                raise ValueError("give params (P, n_params) or n_members")
            p, self.n_members = None, int(n_members)
        else:
            p = _host_block(params, self.n_params, rows=None)
            self.n_members = p.shape[0]
            if n_members is not None and int(n_members) != self.n_members:
                raise ValueError("params has %d rows, n_members is %d" % (self.n_members, n_members))
        self._create(device, self.n_members, None if p is None else p.ctypes.data)

    # ------------------------------------------------------------------ parameters
    def set_params(self, params):
        """All members from a host array (P, n_params); synchronises the device."""
        p = _host_block(params, self.n_params, rows=self.n_members)
        check(self._lib.bsk_population_set_params(self._handle(), p.ctypes.data))

    def set_params_device(self, src, first=0, count=None, stream=0):
        """Members ``first .. first + count - 1`` from DEVICE memory: ``src`` a raw pointer to ``count`` blocks of n_params float32
        (``count`` defaults to the members from ``first`` on), or anything with ``__cuda_array_interface__`` - a contiguous float32
        array of (count, n_params) or count * n_params elements.  One launch on ``stream``: no copy, no synchronisation,
        capturable.  A source array must stay alive until the launch has run."""
        def refuse(typestr, shape, size, dense):
            if typestr != "<f4" or size % self.n_params or size == 0:
                return "device parameters: float32, a multiple of %d elements, got %r %r" % (self.n_params, typestr, shape)
            if not dense:
                return "device parameters must be contiguous"
            if count is not None and int(count) * self.n_params != size:
                return "device parameters: %d members need %d elements, got %d" % (count, int(count) * self.n_params, size)
        src, size = self._device_pointer(src, 4, refuse)
        if count is None:
            count = self.n_members - int(first) if size is None else size // self.n_params
        check(self._lib.bsk_population_set_params_device(self._handle(), C.c_void_p(int(src)) if src else None, int(first), int(count),
                                                         C.c_void_p(int(stream or 0))))

    def set_obs_stats_members(self, n_counted=None):
        """Only the envs of the first ``n_counted`` members feed an attached ``ObsStats`` (None: all of them, the default):
        ``bsk_population_set_obs_stats_members``.  No launch; the next rollout's accumulate launches cover n_counted * E envs."""
        check(self._lib.bsk_population_set_obs_stats_members(self._handle(), self.n_members if n_counted is None else int(n_counted)))

    def set_outcomes(self, rows):
        """Attaches episode-outcome rows (None detaches): ``rows`` is DEVICE memory, float64 (P, 11) - a raw pointer or anything
        with ``__cuda_array_interface__``, the caller's to keep alive.  From then on every rollout also says, per member, how the
        episodes that count ended and which actions they used (``bsk_population_set_outcomes``; ``OUTCOME_COLUMNS``,
        ``population_outcomes_ref``): the value rule's launch at every env step carries the rule, one more small launch follows the
        last step.  The first such rollout of a size allocates and cannot be captured.  No launch, no copy, no synchronisation."""
        ptr = None
        if rows is not None:
            queued = self._source
            ptr, _ = self._device_pointer(rows, 8, _refuse_unless_f64("outcome rows", self.n_members * OUTCOME_COLS))
            self._source = queued                          # (a queued launch still reads its own source)
        check(self._lib.bsk_population_set_outcomes(self._handle(), C.c_void_p(int(ptr)) if ptr else None))
        self._outcomes = rows if ptr else None

    def member(self, m):
        """Member ``m``'s parameter block (n_params,) float32 - what ``DevicePolicy(spec, block)`` takes.  Synchronises."""
        out = np.empty(self.n_params, np.float32)
        check(self._lib.bsk_population_get_member(self._handle(), int(m), out.ctypes.data))
        return out

    # ------------------------------------------------------------------ evaluation
    def act(self, source, envs_per_member=None, mode="greedy", want=("logp", "value", "logits"), env_base=None, stream=None):
        """``DevicePolicy.act`` under the member rule: spacecraft j of ``source`` (a propagator, or a device array (5, n) float64)
        is evaluated with member j // envs_per_member (default n // n_members).  One launch, enqueue-only.  -> the same dict of
        device views."""
        def launch(ptr, stride, n, want, env_base, stream):
            E = n // self.n_members if envs_per_member is None else int(envs_per_member)
            out, outputs = self._outputs(n, want)
            check(self._lib.bsk_population_act(self._handle(), C.c_void_p(ptr), stride, n, E, env_base, MODES[mode], *outputs, n,
                                               C.c_void_p(stream)))
            return out
        return self._act(source, mode, want, env_base, stream, launch)

    def rollout_device(self, prop, n_steps, substeps, mode="greedy", gamma=1.0, d_obs_hist=None, d_reward_hist=None, d_reason_hist=None,
                       d_action_hist=None, d_logp_hist=None, d_value_hist=None, d_env_value=None, d_env_len=None, d_fitness=None,
                       d_mean_len=None, d_outcomes=None):
        """``bsk_population_rollout`` with device pointers (or None): one generation on the propagator's stream - per env step the
        policy launch for every member, the step, and one launch for the history rows and the running values; then the fitness
        (``d_env_value`` f64[n], ``d_env_len`` i32[n], ``d_fitness`` f64[P], ``d_mean_len`` f64[P]).  No copy, no synchronisation;
        capturable after a first rollout of the size has allocated the population's scratch rows.  ``d_outcomes``: f64[P][11] the
        episode-outcome rows are written to - attached for this call (``set_outcomes``), which leaves the population with what it
        had attached before; None: the rollout is passed what it was passed before."""
        if mode not in MODES:
            raise ValueError("mode must be 'greedy' or 'sample'")
        prop = getattr(prop, "propagator", prop)
        vp = lambda p: C.c_void_p(int(p)) if p else None      # noqa: E731

        def launch():
            check(self._lib.bsk_population_rollout(self._handle(), prop._handle(), MODES[mode], int(substeps), int(n_steps), float(gamma),
                                                   vp(d_obs_hist), vp(d_reward_hist), vp(d_reason_hist), vp(d_action_hist),
                                                   vp(d_logp_hist), vp(d_value_hist), vp(d_env_value), vp(d_env_len), vp(d_fitness),
                                                   vp(d_mean_len)))
        if d_outcomes is None:
            return launch()
        before = getattr(self, "_outcomes", None)
        self.set_outcomes(d_outcomes)
        try:
            launch()
        finally:
            self.set_outcomes(before)

    def evaluate(self, prop, n_steps, substeps, mode="greedy", gamma=1.0, outcomes=False):
        """One generation with host results: -> dict ``fitness`` (P,), ``mean_len`` (P,), ``env_value`` (n,) float64 and ``env_len``
        (n,) int32; with ``outcomes`` also ``outcomes``, the members' episode-outcome rows as a dict of (P,) arrays by
        ``OUTCOME_COLUMNS`` (``outcome_table_ref``).  Allocates device scratch per call and synchronises: the convenience form; a
        search loop that keeps its candidates on the device hands ``rollout_device`` its own buffers."""
        prop = getattr(prop, "propagator", prop)
        n, P = prop.n_envs, self.n_members
        host = {"env_value": np.empty(n, np.float64), "env_len": np.empty(n, np.int32), "fitness": np.empty(P, np.float64),
                "mean_len": np.empty(P, np.float64)}
        if outcomes:
            host["outcomes"] = np.empty((P, OUTCOME_COLS), np.float64)
        res = self._host_rollout(prop, host, lambda d: self.rollout_device(prop, n_steps, substeps, mode, gamma,
                                                                           **{"d_" + k: p for k, p in d.items()}))
        if outcomes:
            res["outcomes"] = outcome_table_ref(res["outcomes"])
        return res


def _refuse_unless_f64(noun, count):
    """``_device_pointer``'s ``refuse`` for what must be ``count`` contiguous float64; ``noun`` names it in the message."""
    def refuse(typestr, shape, size, dense):
        if typestr != "<f8" or size != count or (len(shape) == 1 and not dense):       # (a 1-D array's stride only)
            return "%s: %d contiguous float64, got %r %r" % (noun, count, typestr, shape)
    return refuse


class DeviceEvolutionStrategy(_DeviceObject):
    """``EvolutionStrategy``'s search with theta, the ranking and the update on the device (``bsk_es_*``): ``ask`` writes the
    ``population`` = P members straight into a ``PolicyPopulation``'s device layout, ``tell`` reads the P float64 fitness values
    a rollout left in device memory; both are enqueue-only and capturable, and the noise is regenerated from (seed, generation,
    pair, parameter) instead of stored.  ``theta``: the float32 parameter block the search starts from (None: zeros).  Equal bit
    for bit to ``es_ask_ref`` / ``es_tell_ref``.  ``optimizer="adam"`` drives the same estimate through Adam with the L2 penalty
    ``weight_decay`` (``bsk_es_set_optimizer``; ``es_tell_adam_ref``); ``"sgd"``, the default, ignores the four Adam arguments.
    ``sigma_adapt="pgpe"`` gives every parameter a step size of its own in device memory, started at ``sigma`` and adapted by
    every ``tell`` from the same pairs that move theta (``bsk_es_set_sigma_adaptation``; ``es_ask_sigma_ref``,
    ``es_tell_pgpe_ref``): by ``lr_sigma``, at most ``sigma_max_change`` of itself per generation, inside
    [``sigma_min``, ``sigma_max``] (None: ``sigma`` / 100 and 10 ``sigma``).  None, the default, keeps the one ``sigma`` and never
    calls that entry point.  ``log_capacity`` > 0 keeps a training log of that many generations and the best member so far on
    the device (``set_log``; ``training_log``, ``best``); 0, the default, never calls that entry point either.
    ``validation_members`` = V > 0 scores the centre theta on fixed episodes inside every generation (``set_validation``;
    ``validation_log``, ``validated_best``): ``ask`` then takes a population of ``members_total`` = P + V members, the last V
    holding the centre, and ``tell`` P + V fitness values, of which ranking, log, champion and update read the first P; 0, the
    default, never calls that entry point either.  ``set_outcome_log`` adds a third ring, of what the members' episodes did
    (``outcome_log``).  Not thread-safe, one stream at a time."""
    _kind, _what = "es", "evolution strategy"

    def __init__(self, spec, theta, population, sigma=0.1, lr=0.05, seed=0, frozen=10, device=0, optimizer="sgd", beta1=0.9,
                 beta2=0.999, eps=1e-8, weight_decay=0.0, sigma_adapt=None, lr_sigma=0.1, sigma_max_change=0.2, sigma_min=None,
                 sigma_max=None, log_capacity=0, validation_members=0, validation_capacity=None, validation_epoch=0xFFFFFFFF):
        # every argument is checked before the handle exists: a bad one leaves none behind
        log_capacity = check_log(log_capacity)
        check_validation(validation_members, validation_capacity, validation_epoch, log_capacity)
        self.outcome_capacity = 0
        self.optimizer, self.adam = optimizer, self._check_optimizer(optimizer, beta1, beta2, eps, weight_decay)
        self._check_sigma_adapt(sigma_adapt, lr_sigma, sigma_max_change, sigma_min, sigma_max, sigma)
        self.sigma_adapt, self.sigma_adaptation = None, None
        self.log_capacity, self.validation_members, self.validation_capacity, self.validation_epoch = 0, 0, 0, 0
        self._len_ptr, self._len_bound, self._val_masks = None, {}, {}
        self.spec = _as_spec(spec)
        self.n_params = n_params(self.spec)
        self.population, self.sigma, self.lr, self.frozen = int(population), float(sigma), float(lr), int(frozen)
        self.seed = int(seed)
        t = None if theta is None else _host_block(theta, self.n_params)
        self._create(device, self.population, None if t is None else t.ctypes.data, self.sigma, self.lr, self.frozen, self.seed)
        if optimizer == "adam":
            self.set_optimizer("adam", *self.adam)
        if sigma_adapt is not None:
            self.set_sigma_adaptation(sigma_adapt, lr_sigma, sigma_max_change, sigma_min, sigma_max)
        if log_capacity:
            self.set_log(log_capacity)
        if validation_members:
            self.set_validation(validation_members, validation_capacity, validation_epoch)

    def close(self):
        for b in (getattr(self, "_val_masks", None) or {}).values():
            b.free()
        self._val_masks, self._len_bound = {}, {}
        super(DeviceEvolutionStrategy, self).close()

    def _device_word(self, name):
        """``bsk_es_<name>_device`` -> a DEVICE pointer into the optimiser's own memory: no launch, no copy, no synchronisation"""
        p = C.c_void_p()
        check(self._c(name + "_device")(self._handle(), C.byref(p)))
        return p.value

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
        t = None if theta is None else _host_block(theta, self.n_params, np.float64)
        check(self._lib.bsk_es_set_state(self._handle(), None if t is None else t.ctypes.data, int(generation)))

    def generation_ptr(self):
        """The generation counter as a DEVICE uint64 word, valid until ``close``: the epoch of ``reset_from_pool_shared``."""
        return self._device_word("generation")

    @staticmethod
    def _check_optimizer(optimizer, beta1, beta2, eps, weight_decay):
        """-> Adam's four arguments: as floats and by ``check_adam``'s rules under ``"adam"``, as they came under ``"sgd"``"""
        if optimizer not in ("sgd", "adam"):
            raise ValueError("optimizer must be 'sgd' or 'adam', got %r" % (optimizer,))
        return check_adam(beta1, beta2, eps, weight_decay) if optimizer == "adam" else (beta1, beta2, eps, weight_decay)

    def set_optimizer(self, optimizer, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
        """``"adam"``: Adam with an L2 penalty from zero moments (every selection zeroes them); ``"sgd"``: the plain step.  Theta and
        the generation stay; synchronises."""
        adam = tuple(float(x) for x in self._check_optimizer(optimizer, beta1, beta2, eps, weight_decay))
        check(self._lib.bsk_es_set_optimizer(self._handle(), _lib.ES_ADAM if optimizer == "adam" else _lib.ES_SGD, *adam))
        self.optimizer, self.adam = optimizer, adam

    @property
    def moments(self):
        """Adam's (m, v, beta_pow): float64 (n_params,), (n_params,), (2,); synchronises.  An error while the optimiser is SGD."""
        m, v, bp = np.empty(self.n_params, np.float64), np.empty(self.n_params, np.float64), np.empty(2, np.float64)
        check(self._lib.bsk_es_get_moments(self._handle(), m.ctypes.data, v.ctypes.data, bp.ctypes.data))
        return m, v, bp

    def set_moments(self, m=None, v=None, beta_pow=None):
        """New Adam moments (float64 (n_params,) each) and running powers (float64 (2,)); None keeps; synchronises."""
        arrs = [None if a is None else _host_block(a, size, np.float64, what="values")
                for a, size in ((m, self.n_params), (v, self.n_params), (beta_pow, 2))]
        check(self._lib.bsk_es_set_moments(self._handle(), *[None if a is None else a.ctypes.data for a in arrs]))

    @staticmethod
    def _check_sigma_adapt(sigma_adapt, lr_sigma, sigma_max_change, sigma_min, sigma_max, sigma):
        """-> None, or under ``"pgpe"`` the four arguments of ``bsk_es_set_sigma_adaptation`` by ``check_sigma_adaptation``'s rules,
        the bounds defaulting to ``sigma`` / 100 and 10 ``sigma``"""
        if sigma_adapt not in (None, "pgpe"):
            raise ValueError("sigma_adapt must be None or 'pgpe', got %r" % (sigma_adapt,))
        if sigma_adapt is None:
            return None
        sigma_min = 0.01 * float(sigma) if sigma_min is None else sigma_min
        sigma_max = 10.0 * float(sigma) if sigma_max is None else sigma_max
        return check_sigma_adaptation(lr_sigma, sigma_max_change, sigma_min, sigma_max, sigma)

    def set_sigma_adaptation(self, sigma_adapt, lr_sigma=0.1, sigma_max_change=0.2, sigma_min=None, sigma_max=None):
        """``"pgpe"``: a step size per parameter, every entry started at ``sigma`` (every selection fills the vector again);
        None: the one ``sigma`` again.  Theta, the generation and Adam's state stay; synchronises."""
        args = self._check_sigma_adapt(sigma_adapt, lr_sigma, sigma_max_change, sigma_min, sigma_max, self.sigma)
        kind = _lib.ES_SIGMA_FIXED if args is None else _lib.ES_SIGMA_PGPE
        check(self._lib.bsk_es_set_sigma_adaptation(self._handle(), kind, *(args or (0.0, 0.0, 0.0, 0.0))))
        self.sigma_adapt, self.sigma_adaptation = sigma_adapt, args

    @property
    def sigma_vector(self):
        """The step size of every parameter, float64 (n_params,); synchronises.  An error while ``sigma_adapt`` is None."""
        out = np.empty(self.n_params, np.float64)
        check(self._lib.bsk_es_get_sigma(self._handle(), out.ctypes.data))
        return out

    def set_sigma(self, sigma_vec):
        """New step sizes (float64 (n_params,), every entry finite and positive; the first ``frozen`` are carried, not used);
        synchronises.  An error while ``sigma_adapt`` is None."""
        s = _host_block(sigma_vec, self.n_params, np.float64, what="values")
        check(self._lib.bsk_es_set_sigma(self._handle(), s.ctypes.data))

    # ------------------------------------------------------------------ the one length buffer
    def _lengths(self, who=None, count=0, mean_len=None, turn_off=None):
        """The device pointer the length columns read.  There is ONE for the log and the validation, ``_len_ptr``, because the
        rollout of ``run_generation`` writes one array of mean episode lengths: the optimiser's own buffer (``_own_lengths``), or an
        array a caller bound - ``_len_bound`` says through which of ``set_log`` / ``set_validation``, and keeps it alive.
        No argument -> that pointer, None while both are off.  Otherwise ``who`` ("log" | "validation") is being set to read
        ``count`` lengths (0: off) from ``mean_len`` (None: wherever they are), by these rules: an array given while the other of
        the two is on must be the one that one reads; validation does not come on beside a log reading a caller's array of P
        lengths; with nothing given ``who`` reads what the other reads, and with that off the optimiser's own buffer, zeroed (as it
        is whenever the log comes on reading it).  ``turn_off()``, the caller's call of the library with ``who`` off, runs behind
        these refusals and before anything is allocated or written here: the refusal under capture comes from the library.
        -> the pointer ``who`` reads from now on, None: off"""
        if who is None:
            return self._len_ptr if self.log_capacity or self.validation_members else None
        other, other_on = ("validation", self.validation_members) if who == "log" else ("log", self.log_capacity)
        ptr = None
        if count and mean_len is not None:
            queued = self._source
            ptr, _ = self._device_pointer(mean_len, 8, _refuse_unless_f64("mean_len", count))
            self._source = queued                          # (a queued tell still reads its fitness)
            if other_on and int(ptr or 0) != self._len_ptr:
                raise ValueError("mean_len: while %s is on the %s reads the length buffer set_%s bound (the rollout writes one)"
                                 % ("a log" if other == "log" else other, who, other))
        elif count and who == "validation" and other_on and "log" in self._len_bound:
            raise ValueError("the log reads an array of P lengths the caller bound, and the rollout will write P + V: turn the log off, "
                             "give set_validation a mean_len of P + V values, then set_log the same array")
        turn_off()
        self._len_bound.pop(who, None)
        if not count:
            return None
        if mean_len is not None:
            self._len_bound[who] = mean_len                # (every later tell reads it)
        elif other_on:
            ptr = self._len_ptr
        own = (self._out or {}).get("mean_len")
        if ptr is None or (who == "log" and own is not None and ptr == own.ptr):
            ptr = self._own_lengths()
        self._len_ptr = int(ptr or 0) or None
        return self._len_ptr

    _log_len = property(lambda self: self._len_ptr if self.log_capacity else None)
    _val_len = property(lambda self: self._len_ptr if self.validation_members else None)

    def _own_lengths(self):
        """The optimiser's own length buffer, zeroed -> its pointer: P + ``ES_VAL_MAX_MEMBERS`` float64, so that the log and the
        validation read ONE buffer - the rollout writes one - whichever is turned on first and however many members validate."""
        nbytes = 8 * (self.population + ES_VAL_MAX_MEMBERS)
        if self._out is None:
            self._out = {}
        if "mean_len" not in self._out:
            self._out["mean_len"] = _hip.DeviceBuffer(nbytes, self.device)
        ptr = self._out["mean_len"].ptr
        with _hip.device_guard(self.device):
            _hip.check(_hip.runtime().hipMemsetAsync(C.c_void_p(ptr), 0, nbytes, None), "hipMemsetAsync")
        return ptr

    # ------------------------------------------------------------------ the two records: rows and a champion each
    def _champion(self, name, n_words):
        """``bsk_es_get_<name>`` -> (params float32 (n_params,), fitness, generation[, member])"""
        params, words = np.empty(self.n_params, np.float32), (C.c_double(), C.c_uint64(), C.c_int32())[:n_words]
        check(self._c("get_" + name)(self._handle(), params.ctypes.data, *[C.addressof(x) for x in words]))
        return (params,) + tuple(x.value for x in words)

    def _set_champion(self, name, params, *words):
        """``bsk_es_set_<name>``: ``words`` = fitness, generation[, member]; None keeps"""
        p = None if params is None else _host_block(params, self.n_params)
        kinds = ((C.c_double, float), (C.c_uint64, int), (C.c_int32, int))
        words = [None if x is None else ctype(conv(x)) for x, (ctype, conv) in zip(words, kinds)]
        check(self._c("set_" + name)(self._handle(), None if p is None else p.ctypes.data,
                                     *[None if x is None else C.addressof(x) for x in words]))

    def set_log(self, capacity, mean_len=None):
        """A ring of ``capacity`` generations and the best member so far, on the device (``bsk_es_set_log``): from now on every
        ``tell`` writes the generation's row and applies the champion rule in front of its update (``es_log_row_ref``,
        ``es_best_ref``).  Every call with ``capacity`` > 0 starts from an empty log and no champion; 0 turns both off.
        ``mean_len``: P float64 in DEVICE memory the length columns are read from - a raw pointer or anything with
        ``__cuda_array_interface__``, the caller's to keep alive; None: a buffer of the optimiser's own, zeros (so the two columns
        are +0.0, as with nothing bound) until ``run_generation`` has the rollout write the members' mean episode lengths there.
        Theta, the generation, Adam's state and the step sizes stay; synchronises, and cannot be captured."""
        capacity = check_log(capacity)

        def turn_off():
            check(self._lib.bsk_es_set_log(self._handle(), 0, None))
            self.log_capacity = 0
        ptr = self._lengths("log", self.members_total if capacity else 0, mean_len, turn_off)
        if capacity:
            check(self._lib.bsk_es_set_log(self._handle(), capacity, C.c_void_p(ptr) if ptr else None))
            self.log_capacity = capacity

    def training_log(self):
        """The log as a dict of numpy arrays over the generations it holds, sorted by generation (``es_log_table_ref``):
        ``generation``, ``best``, ``worst``, ``sum``, ``sum_sq``, ``count``, ``best_member``, ``len_sum``, ``best_len`` as the
        device stored them, and ``mean`` / ``std`` of the non-NaN members derived here (NaN where ``count`` is 0).  Synchronises.
        An error with no log."""
        gen = np.empty(max(self.log_capacity, 1), np.uint64)
        rows = np.empty((gen.size, 8), np.float64)
        check(self._lib.bsk_es_get_log(self._handle(), gen.ctypes.data, rows.ctypes.data))
        return es_log_table_ref(gen, rows)

    @property
    def best(self):
        """The champion -> (params float32 (n_params,), fitness, generation, member); (zeros, NaN, ``ES_LOG_EMPTY``, -1) while no
        generation has taken.  Synchronises.  An error with no log."""
        return self._champion("best", 3)

    def set_best(self, params=None, fitness=None, generation=None, member=None):
        """A new champion, for a checkpoint that resumes bit for bit; None keeps; synchronises.  An error with no log."""
        self._set_champion("best", params, fitness, generation, member)

    def best_params_ptr(self):
        """The champion's parameter block as a DEVICE pointer to n_params float32, valid until the next ``set_log`` or ``close``:
        ``pop.set_params_device(es.best_params_ptr(), m, 1)`` loads it into a member with no host in between."""
        return self._device_word("best")

    # ------------------------------------------------------------------ validation on fixed episodes
    @property
    def members_total(self):
        """P + V: the members of the population ``ask`` takes and the fitness values ``tell`` takes."""
        return self.population + self.validation_members

    def set_validation(self, members, capacity=None, epoch=0xFFFFFFFF, mean_len=None):
        """``members`` = V in 1..16 validation members holding the centre theta, a ring of ``capacity`` rows (None: the log's
        capacity, or 64) and the validated champion, on the device (``bsk_es_set_validation``; ``es_center_ref``,
        ``es_validate_ref``); 0 turns it off.  Every call with V > 0 starts from an empty ring and no champion.  Member P + v
        restarts its envs under the epoch word ``epoch`` + v, constant from here on; the default keeps member P's slots away from the
        low generation words ``shared_episodes`` uses (the slot rule reads the low 32 bits of the word: with V > 1 member P + v
        then uses the words v - 1).  ``mean_len``: P + V float64 in DEVICE memory, as ``set_log`` takes; None:
        the buffer the log reads (the rollout writes one), the optimiser's own unless an array was bound there.
        What is exact: under ``greedy`` the centre's validation score is a deterministic function of theta - the same bits for the
        same theta in every generation; ``sample`` still draws per global env index and draw counter.  A validation env that
        finishes restarts by the per-env rule; its later episodes do not count, as everywhere.  Training is untouched bit for bit:
        the validation envs restart under their own mask, their observations do not enter ``obs_stats``, and ranking, log, champion
        and update never read their fitness.  Theta, the generation, Adam's state, the step sizes, the log and its champion stay;
        synchronises, and cannot be captured.  ``run_generation`` builds its device masks in the first call after this one."""
        members, capacity, epoch = check_validation(members, capacity, epoch, self.log_capacity)

        def turn_off():
            check(self._lib.bsk_es_set_validation(self._handle(), 0, 0, 0, None))
            for b in self._val_masks.values():
                b.free()
            self.validation_members, self.validation_capacity, self.validation_epoch, self._val_masks = 0, 0, 0, {}
        ptr = self._lengths("validation", self.population + members if members else 0, mean_len, turn_off)
        if members:
            check(self._lib.bsk_es_set_validation(self._handle(), members, capacity, epoch, C.c_void_p(ptr) if ptr else None))
            self.validation_members, self.validation_capacity, self.validation_epoch = members, capacity, epoch

    def validation_log(self):
        """The validation ring as a dict of numpy arrays over the generations it holds, sorted by generation
        (``es_validation_table_ref``): ``generation``, ``fitness`` (f_c, the centre's mean over its V members), ``mean_len``,
        ``take``, ``members``.  Synchronises.  An error with validation off."""
        gen = np.empty(max(self.validation_capacity, 1), np.uint64)
        rows = np.empty((gen.size, 4), np.float64)
        check(self._lib.bsk_es_get_validation_log(self._handle(), gen.ctypes.data, rows.ctypes.data))
        return es_validation_table_ref(gen, rows)

    @property
    def validated_best(self):
        """The validated champion -> (params float32 (n_params,), fitness, generation): the centre with the best validation score so
        far; (zeros, NaN, ``ES_LOG_EMPTY``) while no generation has taken.  Synchronises.  An error with validation off."""
        return self._champion("validated_best", 2)

    def set_validated_best(self, params=None, fitness=None, generation=None):
        """A new validated champion, for a checkpoint that resumes bit for bit; None keeps; synchronises."""
        self._set_champion("validated_best", params, fitness, generation)

    def validated_best_params_ptr(self):
        """The validated champion's parameter block as a DEVICE pointer to n_params float32, valid until the next ``set_validation``
        or ``close``: what ``pop.set_params_device`` takes."""
        return self._device_word("validated_best")

    def validation_epochs_ptr(self):
        """The V epoch words as a DEVICE pointer to uint64[V], valid until the next ``set_validation`` or ``close``: member P + v's
        ``reset_from_pool_shared`` takes this pointer + 8 v."""
        return self._device_word("validation_epochs")

    def _validation_masks(self, n_envs):
        """The device masks of ``run_generation`` for a handle of ``n_envs`` -> pointer to uint8[1 + V][n_envs]: row 0 the envs of
        the P training members, row 1 + v those of validation member v.  Built and uploaded once per size (it allocates and
        synchronises: the warming call), so that a later call stays capturable."""
        buf = self._val_masks.get(n_envs)
        if buf is None:
            P, V = self.population, self.validation_members
            E = n_envs // (P + V)
            if E < 1 or E * (P + V) != n_envs:
                raise ValueError("the propagator's n_envs (%d) must be a multiple of population + validation_members (%d)" % (n_envs, P + V))
            host = np.zeros((1 + V, n_envs), np.uint8)
            host[0, :P * E] = 1
            for v in range(V):
                host[1 + v, (P + v) * E:(P + v + 1) * E] = 1
            buf = _hip.DeviceBuffer(host.nbytes, self.device)
            with _hip.device_guard(self.device):
                _hip.check(_hip.runtime().hipMemcpyAsync(C.c_void_p(buf.ptr), C.c_void_p(host.ctypes.data), host.nbytes,
                                                         _hip.hipMemcpyHostToDevice, None), "hipMemcpyAsync")
            self.sync()                                    # (the copy reads `host`)
            self._val_masks[n_envs] = buf
        return buf.ptr

    # ------------------------------------------------------------------ episode outcomes
    def set_outcome_log(self, capacity):
        """A ring of ``capacity`` generations of episode outcomes on the device (``bsk_es_set_outcome_log``): from now on
        ``run_generation`` has the rollout write every member's outcome row into a buffer of the optimiser's own
        (``outcomes_ptr``: P + ``ES_VAL_MAX_MEMBERS`` rows, whatever validation is set to later) and every ``tell`` writes, in one
        more launch in front of its update, the totals over the P ranked members, the row of the member the ranking puts first
        and the totals over the validation members (``es_outcome_row_ref``).  Every call with ``capacity`` > 0 starts from an
        empty ring; 0 turns it off.  Everything else of the optimiser stays; synchronises, and cannot be captured."""
        capacity = check_outcome_log(capacity)
        # Off first, as ``_lengths`` turns its record off first: under a capture the library refuses here, BEFORE the allocation and
        # the null-stream memset below, either of which would invalidate the capture.  It costs a second synchronisation, at set-up.
        check(self._lib.bsk_es_set_outcome_log(self._handle(), 0, None))
        self.outcome_capacity = 0
        if not capacity:
            return
        nbytes = 8 * OUTCOME_COLS * (self.population + ES_VAL_MAX_MEMBERS)
        if self._out is None:
            self._out = {}
        if "outcomes" not in self._out:
            self._out["outcomes"] = _hip.DeviceBuffer(nbytes, self.device)
        ptr = self._out["outcomes"].ptr
        with _hip.device_guard(self.device):
            _hip.check(_hip.runtime().hipMemsetAsync(C.c_void_p(ptr), 0, nbytes, None), "hipMemsetAsync")
        check(self._lib.bsk_es_set_outcome_log(self._handle(), capacity, C.c_void_p(ptr)))
        self.outcome_capacity = capacity

    def outcomes_ptr(self):
        """The members' outcome rows as a DEVICE pointer to float64 (P + V, 11), valid until ``close``: what ``run_generation``
        hands the rollout as ``d_outcomes`` and ``tell`` reads.  None while the ring is off."""
        return self._out["outcomes"].ptr if self.outcome_capacity else None

    def outcome_log(self):
        """The ring as a dict over the generations it holds, sorted by generation (``es_outcome_table_ref``): ``generation``, and
        ``members`` (totals over the P ranked members), ``best`` (the first-ranked member's row), ``validation`` (totals over the
        validation members; zeros with validation off) - each a dict of arrays by ``OUTCOME_COLUMNS``.  Synchronises.  An error
        with the ring off."""
        gen = np.empty(max(self.outcome_capacity, 1), np.uint64)
        rows = np.empty((gen.size, 3 * OUTCOME_COLS), np.float64)
        check(self._lib.bsk_es_get_outcome_log(self._handle(), gen.ctypes.data, rows.ctypes.data))
        return es_outcome_table_ref(gen, rows)

    # ------------------------------------------------------------------ the search
    def ask(self, pop, stream=0):
        """This generation's members into every member of ``pop`` (a ``PolicyPopulation`` of the same spec and ``members_total``
        members): one launch on ``stream`` - and one more for the V validation members - no copy, no synchronisation."""
        check(self._lib.bsk_es_ask(self._handle(), pop._handle(), C.c_void_p(int(stream or 0))))

    def tell(self, d_fitness, stream=0):
        """``d_fitness``: P float64 in DEVICE memory (greater is better; P + V while validation is on) - a raw pointer or anything
        with ``__cuda_array_interface__``.  Ranks the first P, moves theta and advances the generation: three launches on
        ``stream``, with a log on two more in front of the update, with validation on two more behind those, and with the
        outcome ring on one more behind those."""
        d_fitness, _ = self._device_pointer(d_fitness, 8, _refuse_unless_f64("device fitness", self.members_total))
        check(self._lib.bsk_es_tell(self._handle(), C.c_void_p(int(d_fitness)) if d_fitness else None, C.c_void_p(int(stream or 0))))

    def fitness_buffer(self):
        """The device buffer of P float64 (P + V while validation is on) ``run_generation`` has the rollout write the fitness to
        (``_hip.DeviceBuffer``)."""
        if self._out is None:
            self._out = {}
        want = 8 * self.members_total
        if "fitness" in self._out and self._out["fitness"].nbytes < want:
            self.sync()                                    # (a queued tell still reads the smaller one)
            self._out.pop("fitness").free()
        if "fitness" not in self._out:
            self._out["fitness"] = _hip.DeviceBuffer(want, self.device)
        return self._out["fitness"]

    def apply_obs_norm(self, stats, std_min=1e-6, stream=0):
        """theta[0:5] = in_scale, theta[5:10] = in_shift out of ``stats``' totals (``obs_norm_ref``): one launch on ``stream``, no
        copy, no synchronisation.  A row whose standard deviation is below ``std_min`` gets scale 0; nothing is written while
        nothing has been counted.  Needs ``frozen >= 10``; the next ``ask`` carries the ten floats into every member."""
        check(self._lib.bsk_es_apply_obs_norm(self._handle(), stats._handle(), float(std_min), C.c_void_p(int(stream or 0))))

    def run_generation(self, prop, pop, n_steps, substeps, mode="greedy", gamma=1.0, reset=True, shared_episodes=False, obs_stats=None,
                       std_min=1e-6):
        """One generation on the propagator's stream: every env restarted from the propagator's IC pool (``reset``; needs an
        auto-reset pool), ``ask``, ``pop.rollout_device`` with the fitness into ``fitness_buffer()``, ``tell``.  Nothing else is
        issued - no copy, no synchronisation - so after one warming call (it allocates the buffer and the population's scratch
        rows) a call can be captured into a graph and replayed generation after generation.  ``shared_episodes``: the reset is
        ``reset_from_pool_shared`` with E = n_envs // population and the generation word as the epoch, so that all members of a
        generation are scored on the same E initial conditions and every generation draws new ones; nothing else in the stream
        changes.  That is exact for ``greedy``: sample mode still draws its uniform per global env index.
        ``obs_stats``: an ``ObsStats`` the rollout accumulates into (attached to ``pop`` for the rollout, which is left with what it
        had attached before), and ``apply_obs_norm(obs_stats, std_min)`` behind ``tell``: generation g runs with the statistics of
        the generations before it.  With a log on the rollout also writes the members' mean episode lengths into the buffer
        ``set_log`` bound, for the row's length columns; with it off the rollout is passed what it was passed before.
        With validation on (``set_validation``) ``pop`` has P + V members and E = n_envs // (P + V): the training envs restart as
        above, but under a device mask of the first P * E envs; then validation member v's E envs restart by
        ``reset_from_pool_shared`` under its own mask and its own constant epoch word - one launch each.  The masks are built in
        the first call for a handle's size (the warming call).  ``obs_stats`` counts the first P members only
        (``pop.set_obs_stats_members``; the population is left counting all), and the rollout writes P + V fitness values and
        lengths.  With the outcome ring on (``set_outcome_log``) the rollout also writes the members' outcome rows into
        ``outcomes_ptr()`` (attached to ``pop`` for the rollout, which is left with what it had attached before); with it off the
        rollout is passed what it was passed before."""
        prop = getattr(prop, "propagator", prop)
        fit = self.fitness_buffer()
        stream = prop.stream_ptr()
        V = self.validation_members
        lengths = self._lengths()                          # (None with neither the log nor validation on: as not passed)
        rows = self.outcomes_ptr()                         # (None with the outcome ring off: as not passed)
        if V:
            E = prop.n_envs // self.members_total
            masks = self._validation_masks(prop.n_envs)
            if reset and shared_episodes:
                prop.reset_from_pool_shared(E, self.generation_ptr(), masks)
            elif reset:
                prop.reset_from_pool_device(masks)
            if reset:
                epochs = self.validation_epochs_ptr()
                for v in range(V):
                    prop.reset_from_pool_shared(E, epochs + 8 * v, masks + (1 + v) * prop.n_envs)
        elif reset and shared_episodes:
            prop.reset_from_pool_shared(prop.n_envs // self.population, self.generation_ptr())
        elif reset:
            prop.reset_from_pool_device(None)
        self.ask(pop, stream)
        if obs_stats is None:
            pop.rollout_device(prop, n_steps, substeps, mode, gamma, d_fitness=fit.ptr, d_mean_len=lengths, d_outcomes=rows)
            self.tell(fit.ptr, stream)
            return
        before = getattr(pop, "_stats", None)
        pop.set_obs_stats(obs_stats)
        if V:
            pop.set_obs_stats_members(self.population)
        try:
            pop.rollout_device(prop, n_steps, substeps, mode, gamma, d_fitness=fit.ptr, d_mean_len=lengths, d_outcomes=rows)
        finally:
            if V:
                pop.set_obs_stats_members(None)
            pop.set_obs_stats(before)
        self.tell(fit.ptr, stream)
        self.apply_obs_norm(obs_stats, std_min, stream)
