"""Batched lookahead planning on the GPU: "plan, then act" for thousands of spacecraft without a host visit.

``LookaheadPlanner`` forks every root env into ``3**depth`` branches (``bsk_fork_device``), rolls every branch out under its own
action sequence for ``depth + tail_steps`` env steps (``bsk_step_n``) and picks, per root, the first action of the branch with the
greatest discounted return (``bsk_select_branches``).  Branch b takes base-3 digit t of b at step t < depth, then ``tail_action``;
the branch's return stops after the first step that ends its episode (that step's reward and penalty included).  All three are
enqueued on the root's stream from buffers built once, so ``plan()`` - and a step of the root on the planned actions - can be
captured into one HIP graph.  An extra beside the reference surface: the reference has no forking or planning.

``BeamPlanner`` looks further ahead than 3**depth branches allow: per root it keeps the ``width`` best action sequences, and every
level forks them into their 3 children (``bsk_fork_device``), steps the children once (``bsk_step_device``), keeps the ``width``
best children (``bsk_beam_select``) and forks them back, so its cost grows linearly with the ``horizon``.

Both cut every sequence off at their horizon and score the rest of the episode as zero - unless they are given a ``value_policy``,
a ``DevicePolicy`` with a value network: one more launch (``bsk_policy_value``) then evaluates it on the observations the sequences
end in, and the choice adds its discounted estimate to every sequence whose episode has not ended (``bsk_select_branches_boot``,
``bsk_beam_select_boot``): n-step lookahead with a learned value at the leaf.  ``distill(..., value_targets=True)`` on such a planner
fits the value network to n-step targets formed through the planner's own max, which makes distillation an iteration.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FLAG_AUTO_RESET, FLAG_EPISODE_STATS, FLAG_LDS_SCRATCH, FLAG_OBS_ROWMAJOR, GRAV_SH, check

MAX_DEPTH = 6
MAX_WIDTH = 81                  # BSK_BEAM_MAX_WIDTH: 3 * width candidates of a root fit one 256-thread workgroup
# bsk_beam_slot (include/bskgpu.h): one beam entry; flags bit 0 valid, bit 1 live
BEAM_SLOT = np.dtype([("value", "<f8"), ("first", "<i4"), ("flags", "<u4")])
BEAM_VALID, BEAM_LIVE = 1, 2
# the flags a branch handle drops: they change what a step writes or the kernel's form, never its arithmetic (bsk_fork_device)
BRANCH_CLEARED_FLAGS = FLAG_AUTO_RESET | FLAG_EPISODE_STATS | FLAG_OBS_ROWMAJOR | FLAG_LDS_SCRATCH


def check_args(n_roots, depth, tail_steps, tail_action, gamma):
    """Argument rules of ``LookaheadPlanner`` (no device needed) -> n_branch."""
    if not (isinstance(depth, (int, np.integer)) and 1 <= depth <= MAX_DEPTH):
        raise ValueError("depth must be an integer in 1..%d" % MAX_DEPTH)
    if not (isinstance(tail_steps, (int, np.integer)) and tail_steps >= 0):
        raise ValueError("tail_steps must be a non-negative integer")
    if tail_action not in (0, 1, 2):
        raise ValueError("tail_action must be 0, 1 or 2")
    if not np.isfinite(gamma):
        raise ValueError("gamma must be finite")
    n_branch = int(n_roots) * 3 ** int(depth)
    if n_branch >= 2 ** 31:
        raise ValueError("n_roots * 3**depth = %d branches: must stay below 2**31" % n_branch)
    return n_branch


def action_table(n_roots, depth, tail_steps=0, tail_action=0):
    """int32[depth + tail_steps][n_roots * 3**depth]: branch b takes base-3 digit t of b at step t < depth, ``tail_action`` after.
    (b = root * 3**depth + local index, so digit t of b is digit t of the local index.)"""
    b = np.arange(int(n_roots) * 3 ** int(depth), dtype=np.int64)
    rows = [(b // 3 ** t) % 3 for t in range(depth)] + [np.full_like(b, tail_action) for _ in range(tail_steps)]
    return np.ascontiguousarray(np.stack(rows).astype(np.int32))


def fork_map(n_roots, depth):
    """int32[n_roots * 3**depth]: branch j is a copy of root j // 3**depth."""
    return (np.arange(int(n_roots) * 3 ** int(depth), dtype=np.int64) // 3 ** int(depth)).astype(np.int32)


def branch_values(reward_hist, reason_hist, gamma):
    """numpy restatement of bsk_select_branches' branch value (include/bskgpu.h), same operations in the same order:
    v = v + g * r[t]; g = g * gamma, stopping after the first t with reason[t] != 0."""
    r = np.asarray(reward_hist, dtype=np.float64)
    q = np.asarray(reason_hist)
    v = np.zeros(r.shape[1])
    g = np.ones(r.shape[1])
    live = np.ones(r.shape[1], dtype=bool)
    for t in range(r.shape[0]):
        v = np.where(live, v + g * r[t], v)
        g = g * gamma
        live &= q[t] == 0
    return v


def branch_values_boot(reward_hist, reason_hist, gamma, leaf):
    """numpy restatement of bsk_select_branches_boot's branch value (include/bskgpu.h), same operations in the same order:
    ``branch_values``' loop, then v = v + g * leaf for the branches no step ended (g after ``n_steps`` multiplications; product,
    then sum); a branch that ended - at the last step too - keeps its value."""
    r = np.asarray(reward_hist, dtype=np.float64)
    q = np.asarray(reason_hist)
    v = np.zeros(r.shape[1])
    g = np.ones(r.shape[1])
    live = np.ones(r.shape[1], dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(r.shape[0]):
            v = np.where(live, v + g * r[t], v)
            g = g * gamma
            live &= q[t] == 0
        return np.where(live, v + g * np.asarray(leaf, dtype=np.float32).astype(np.float64), v)


def select_best(values, group):
    """Best branch of every group of ``group`` consecutive values: greatest value, ties to the lowest index, NaN loses to every
    number (a group of NaNs picks index 0) -> (index within the group int64[n_groups], value f64[n_groups])."""
    v = np.asarray(values, dtype=np.float64).reshape(-1, int(group))
    key = np.where(np.isnan(v), -np.inf, v)
    best = np.argmax(key, axis=1)                                       # first occurrence of the maximum: the lowest index
    # a NaN must lose to -inf too: where the winner is a NaN (-inf key) but a real -inf exists, take the first real -inf
    nan_win = np.isnan(v[np.arange(v.shape[0]), best])
    if nan_win.any():
        real = ~np.isnan(v)
        has_real = real.any(axis=1)
        first_real = np.argmax(real, axis=1)
        best = np.where(nan_win & has_real, first_real, np.where(nan_win, 0, best))
    return best, v[np.arange(v.shape[0]), best]


def check_beam_args(n_roots, width, horizon, gamma):
    """Argument rules of ``BeamPlanner`` (no device needed) -> the level weights w_t, f64[horizon]."""
    if not (isinstance(width, (int, np.integer)) and 1 <= width <= MAX_WIDTH):
        raise ValueError("width must be an integer in 1..%d" % MAX_WIDTH)
    if not (isinstance(horizon, (int, np.integer)) and horizon >= 1):
        raise ValueError("horizon must be a positive integer")
    if not np.isfinite(gamma):
        raise ValueError("gamma must be finite")
    if 3 * int(width) * int(n_roots) >= 2 ** 31:
        raise ValueError("3 * width * n_roots = %d children: must stay below 2**31" % (3 * int(width) * int(n_roots)))
    w = level_weights(gamma, horizon)
    if not np.isfinite(w).all():
        raise ValueError("gamma**t overflows within the horizon")
    return w


def level_weights(gamma, horizon):
    """w_0 = 1, w_t = w_{t-1} * gamma: the factors bsk_select_branches applies to step t, rounded in the same order."""
    w, out = 1.0, []
    for _ in range(int(horizon)):
        out.append(w)
        w = w * float(gamma)
    return np.array(out)


def beam_candidates(reward, reason, n_roots, width, level, weight, slots_in=None):
    """The 3 * width * n_roots candidates of one beam level (bsk_beam_select, include/bskgpu.h) -> BEAM_SLOT[]: candidate c is
    child c % 3 of slot c // 3.  Level 0 ignores ``slots_in``: only slot 0 of each root is a parent.  Later levels: valid iff the
    parent is valid and live, or the action is 0 (a finished sequence continues as one candidate); value = value[p] + w * r[c]
    while the parent is live (product, then sum), else value[p].  Invalid candidates: value NaN, first -1, flags 0."""
    n = 3 * int(width) * int(n_roots)
    r = np.asarray(reward, dtype=np.float64)[:n]
    q = np.asarray(reason)[:n]
    c = np.arange(n)
    p, a = c // 3, c % 3
    with np.errstate(invalid="ignore", over="ignore"):
        if level == 0:
            valid = p % int(width) == 0
            live = q == 0
            value = np.float64(0.0) + weight * r
            first = a
        else:
            par = np.asarray(slots_in).view(BEAM_SLOT)[p]
            p_live = (par["flags"] & BEAM_LIVE) != 0
            valid = ((par["flags"] & BEAM_VALID) != 0) & (p_live | (a == 0))
            live = p_live & (q == 0)
            value = np.where(p_live, par["value"] + weight * r, par["value"])
            first = par["first"]
    out = np.zeros(n, dtype=BEAM_SLOT)
    out["value"] = np.where(valid, value, np.nan)
    out["first"] = np.where(valid, first, -1)
    out["flags"] = np.where(valid, BEAM_VALID | np.where(live, BEAM_LIVE, 0), 0)
    return out


def beam_order(cand, n_roots):
    """Candidate indices of every root in rank order -> int64[n_roots][3 * width]: valid before invalid; valid ones by the greater
    value, NaN after every number, equal values to the lower index (select_best's rule); invalid ones by index."""
    n = len(cand)
    c = np.arange(n)
    valid = (cand["flags"] & BEAM_VALID) != 0
    key = np.where(valid, -cand["value"], 0.0)             # (ascending sorts put NaN last; -0.0 and 0.0 compare equal)
    return np.lexsort((c, key, ~valid, c // (n // int(n_roots)))).reshape(int(n_roots), -1)


def beam_select_ref(reward, reason, n_roots, width, level, weight, slots_in=None):
    """numpy restatement of one ``bsk_beam_select`` level (include/bskgpu.h), bit for bit -> (slots_out BEAM_SLOT[n_roots * width],
    map int32[n_roots * width], best_value f64[n_roots], best_action int32[n_roots])."""
    cand = beam_candidates(reward, reason, n_roots, width, level, weight, slots_in)
    keep = beam_order(cand, n_roots)[:, :int(width)].ravel()
    out = cand[keep]
    fmap = np.where((out["flags"] & BEAM_VALID) != 0, keep, -1).astype(np.int32)
    return out, fmap, out["value"][::int(width)].copy(), out["first"][::int(width)].copy()


def beam_keys(cand, leaf, boot_weight):
    """What bsk_beam_select_boot ranks the candidates ``cand`` (``beam_candidates``) by -> f64[]: value + boot_weight * leaf
    (product, then sum) for a valid candidate that is live after this step, its value for a valid one that is not, NaN for an
    invalid one."""
    live = (cand["flags"] & BEAM_LIVE) != 0
    lf = np.asarray(leaf, dtype=np.float32)[:len(cand)].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(live, cand["value"] + np.float64(boot_weight) * lf, cand["value"])


def beam_select_boot_ref(reward, reason, leaf, n_roots, width, level, weight, boot_weight, slots_in=None):
    """numpy restatement of one ``bsk_beam_select_boot`` level (include/bskgpu.h), bit for bit -> (slots_out BEAM_SLOT[n_roots *
    width] with the UN-bootstrapped values, map int32[n_roots * width], keys f64[n_roots * width], best_value f64[n_roots] - the
    key of rank 0 -, best_action int32[n_roots])."""
    cand = beam_candidates(reward, reason, n_roots, width, level, weight, slots_in)
    keys = beam_keys(cand, leaf, boot_weight)
    ranked = cand.copy()
    ranked["value"] = keys                                 # (beam_order's rule with the key in place of the value)
    keep = beam_order(ranked, n_roots)[:, :int(width)].ravel()
    out = cand[keep]
    fmap = np.where((out["flags"] & BEAM_VALID) != 0, keep, -1).astype(np.int32)
    return out, fmap, keys[keep], keys[keep][::int(width)].copy(), out["first"][::int(width)].copy()


def check_bootstrap(bootstrap):
    """Argument rule of ``BeamPlanner(bootstrap=...)`` (no device needed)."""
    if bootstrap not in ("every", "last"):
        raise ValueError("bootstrap must be 'every' or 'last', got %r" % (bootstrap,))
    return bootstrap


def check_value_policy(value_policy, device=None):
    """Argument rules of a planner's ``value_policy`` (no device needed): None, or a ``DevicePolicy`` with a value network - on
    ``device`` where one is given."""
    if value_policy is None:
        return None
    spec = getattr(value_policy, "spec", None)
    if spec is None or not hasattr(value_policy, "value_enqueue"):
        raise TypeError("value_policy must be a DevicePolicy, got %r" % type(value_policy))
    if spec.value_hidden is None:
        raise ValueError("value_policy: the policy has no value network")
    if device is not None and value_policy.device != device:
        raise ValueError("value_policy lives on device %d, the root on device %d" % (value_policy.device, device))
    return value_policy


class _BranchPlanner(object):
    """What both planners share: the root checks, branch handles on the root's device and stream (the root's config minus
    ``BRANCH_CLEARED_FLAGS``, its sim time and spherical-harmonic field), device buffers built once, and reading them back."""
    _handle_names = ()

    def _attach(self, root, substeps):
        from .simulators.dynamics import BatchedPropagator
        prop = getattr(root, "propagator", root)
        if substeps is None:
            substeps = getattr(root, "substeps", None)
        if not isinstance(prop, BatchedPropagator):
            raise TypeError("%s needs a BatchedPropagator or a LeoPowerAttVecEnv over one (sharded propagators are not "
                            "supported: fork within each shard)" % type(self).__name__)
        if substeps is None or int(substeps) < 1:
            raise ValueError("substeps (RK4 steps per env step) is required for a BatchedPropagator root")
        self.root, self.substeps, self.n_roots = prop, int(substeps), int(prop.n_envs)
        self._buffers = []

    def _open(self, sizes):
        """Creates the branch handles ``sizes`` names ((attribute, n_envs) pairs), then ``_build()``."""
        from .simulators.dynamics import BatchedPropagator
        prop = self.root
        if prop.cfg.gravity_model == GRAV_SH and prop.gravity_sh is None:
            raise ValueError("the root has no spherical-harmonic field yet (set_gravity_sh)")
        cfg = prop.cfg.copy()
        cfg.flags &= ~BRANCH_CLEARED_FLAGS
        self.stream = prop.stream_ptr()
        try:
            for name, n in sizes:
                h = BatchedPropagator(cfg, n, device=prop.device, stream=self.stream)
                setattr(self, name, h)
                if prop.sim_time:
                    h.set_sim_time(prop.sim_time)
                if prop.gravity_sh is not None:
                    h.set_gravity_sh(*prop.gravity_sh)
            self._build()
        except BaseException:
            self.close()
            raise

    def _dev(self, nbytes, host=None):
        from . import _hip
        b = _hip.DeviceBuffer(max(int(nbytes), 1), self.root.device)
        self._buffers.append(b)
        if host is not None:
            host = np.ascontiguousarray(host)
            rt = _hip.runtime()
            _hip.check(rt.hipMemcpyAsync(C.c_void_p(b.ptr), C.c_void_p(host.ctypes.data), host.nbytes, _hip.hipMemcpyHostToDevice,
                                         C.c_void_p(self.stream)), "hipMemcpyAsync")
            _hip.stream_sync(self.stream)              # (pageable source: the copy must be done before `host` goes)
        return b

    def _read(self, buf, dtype, count):
        from . import _hip
        out = np.empty(count, dtype=dtype)
        _hip.check(_hip.runtime().hipMemcpyAsync(C.c_void_p(out.ctypes.data), C.c_void_p(buf.ptr), out.nbytes, _hip.hipMemcpyDeviceToHost,
                                                 C.c_void_p(self.stream)), "hipMemcpyAsync")
        self.root.sync()
        for name in self._handle_names:
            getattr(self, name).sync()  # (reports a fork's device error, if any)
        return out

    def _actions_view(self):
        from .simulators.dynamics.propagator import _DevArray
        return _DevArray(self.d_best_action.ptr, (self.n_roots,), "<i4", owner=self.root, device=self.root.device, stream=self.stream)

    def plan_host(self):
        """``plan()``, then -> (actions int32 (n_roots,), values f64 (n_roots,)) on the host (synchronises)."""
        self.plan()
        return self.last_actions(), self.last_values()

    def last_actions(self):
        return self._read(self.d_best_action, np.int32, self.n_roots)

    def last_values(self):
        """best value per root of the last plan (the best branch's, or the best kept sequence's)"""
        return self._read(self.d_best_value, np.float64, self.n_roots)

    def close(self):
        for name in self._handle_names:
            h = getattr(self, name, None)
            if h is not None:
                h.sync()
                h.close()
                setattr(self, name, None)
        for b in getattr(self, "_buffers", []):
            b.free()
        self._buffers = []


class LookaheadPlanner(_BranchPlanner):
    """Exhaustive lookahead of ``depth`` env steps (3**depth branches per root), then ``tail_steps`` steps of ``tail_action``.

    ``root``: a ``BatchedPropagator`` (``substeps`` required) or a ``LeoPowerAttVecEnv`` (its ``propagator`` and ``substeps``).
    The planner owns a branch propagator of ``n_roots * 3**depth`` envs on the root's device and stream with the root's config
    minus ``BRANCH_CLEARED_FLAGS``, the root's sim time and spherical-harmonic field, and device buffers built once: the fork map,
    the action table, the histories and the outputs.  A later ``set_sim_time`` / ``set_gravity_sh`` on the root needs a new planner
    (the fork refuses partners that differ).

    ``value_policy``: a ``DevicePolicy`` with a value network on the root's device (None: the plain planner, launch for launch).
    Every branch no step ended then adds ``gamma**n_steps`` times the value network's estimate of its last observation
    (``branch_values_boot``): ``last_values()``, ``last_branch_values()`` and ``d_best_value`` carry bootstrapped estimates.  The
    policy is read, not owned; its parameters may change between plans (``PolicyFit``), which is what makes ``distill`` on such a
    planner an iteration."""
    _handle_names = ("branch",)

    def __init__(self, root, depth=2, tail_steps=0, tail_action=0, gamma=1.0, substeps=None, value_policy=None):
        check_value_policy(value_policy)
        self._attach(root, substeps)
        self.value_policy = check_value_policy(value_policy, self.root.device)
        self.n_branch = check_args(self.n_roots, depth, tail_steps, tail_action, gamma)
        self.depth, self.tail_steps, self.tail_action, self.gamma = int(depth), int(tail_steps), int(tail_action), float(gamma)
        self.group = 3 ** self.depth
        self.n_steps = self.depth + self.tail_steps
        self._open([("branch", self.n_branch)])

    def _build(self):
        nb, T = self.n_branch, self.n_steps
        table = action_table(self.n_roots, self.depth, self.tail_steps, self.tail_action)
        self.d_map = self._dev(4 * nb, fork_map(self.n_roots, self.depth))
        self.d_actions = self._dev(4 * nb * T, table)
        self.d_first_action = self._dev(4 * nb, table[0])
        self.d_reward_hist = self._dev(8 * nb * T)
        self.d_reason_hist = self._dev(nb * T)
        self.d_values = self._dev(8 * nb)
        self.d_best_value = self._dev(8 * self.n_roots)
        self.d_best_action = self._dev(4 * self.n_roots)
        if self.value_policy is not None:
            views = self.branch.device_views()
            self._d_obs, self._obs_stride = views["obs"].__cuda_array_interface__["data"][0], views["stride"]
            self.d_leaf = self._dev(4 * nb)                                  # f32[n_branch]: the value network at every leaf

    def plan(self):
        """fork -> ``depth + tail_steps`` env steps of every branch -> per-root choice, all enqueued on the root's stream (no copy,
        no synchronisation).  With a ``value_policy``: its value network on the branches' last observations (``bsk_policy_value``)
        in front of the choice, which then adds the discounted leaf value to every branch no step ended
        (``bsk_select_branches_boot``).  -> int32 (n_roots,) device view of the chosen actions (``__cuda_array_interface__`` / DLPack):
        ``root.step_device(view.__cuda_array_interface__["data"][0], ...)`` and ``torch.from_dlpack(view)`` take it as it is."""
        self.branch.fork_from(self.root, self.d_map.ptr)
        self.branch.step_n(self.n_steps, self.substeps, self.d_actions.ptr, d_reward_hist=self.d_reward_hist.ptr,
                           d_reason_hist=self.d_reason_hist.ptr)
        if self.value_policy is not None:
            self.value_policy.value_enqueue(self._d_obs, self._obs_stride, self.n_branch, self.d_leaf.ptr, self.stream)
            check(_lib.load().bsk_select_branches_boot(C.c_void_p(self.d_reward_hist.ptr), C.c_void_p(self.d_reason_hist.ptr),
                                                       C.c_void_p(self.d_first_action.ptr), self.n_steps, self.n_branch, self.group,
                                                       self.gamma, C.c_void_p(self.d_leaf.ptr), C.c_void_p(self.d_values.ptr),
                                                       C.c_void_p(self.d_best_value.ptr), C.c_void_p(self.d_best_action.ptr),
                                                       C.c_void_p(self.stream)))
            return self._actions_view()
        check(_lib.load().bsk_select_branches(C.c_void_p(self.d_reward_hist.ptr), C.c_void_p(self.d_reason_hist.ptr),
                                              C.c_void_p(self.d_first_action.ptr), self.n_steps, self.n_branch, self.group, self.gamma,
                                              C.c_void_p(self.d_values.ptr), C.c_void_p(self.d_best_value.ptr),
                                              C.c_void_p(self.d_best_action.ptr), C.c_void_p(self.stream)))
        return self._actions_view()

    def last_branch_values(self):
        """value of every branch of the last plan, f64 (n_roots, 3**depth)"""
        return self._read(self.d_values, np.float64, self.n_branch).reshape(self.n_roots, self.group)


class BeamPlanner(_BranchPlanner):
    """Beam search over ``horizon`` env steps, keeping the ``width`` best action sequences of every root (bsk_beam_select).

    ``root`` as for ``LookaheadPlanner`` (same refusals).  The planner owns two branch propagators on the root's stream: ``beam``
    (``n_roots * width`` envs, the kept sequences: slot s belongs to root s // width) and ``children`` (``3 * width * n_roots``
    envs: child c is slot c // 3 after action c % 3), and builds every device buffer once.  ``plan()`` forks the root into every
    slot, then per level forks the slots into their children, steps the children once, keeps the ``width`` best children of every
    root and forks them back into the slots (not after the last level): 4 * horizon launches, capturable into one HIP graph.
    A sequence whose episode has ended continues with action 0 alone and keeps its value.  With ``width >= 3**horizon`` the
    best value equals ``LookaheadPlanner(depth=horizon)``'s bit for bit; ``width == 1`` is a greedy one-step lookahead.  Without
    ``FLAG_DESAT`` actions 1 and 2 command the same thing: their children tie exactly and both take a slot.

    ``value_policy``: a ``DevicePolicy`` with a value network on the root's device (None: the plain planner, launch for launch).
    A level then runs the value network on the children's observations (``bsk_policy_value``, a fifth launch) and ranks them by
    "return so far + ``w_{t+1}`` times the value of where they stand" (``bsk_beam_select_boot``; an ended sequence by its return
    alone); the slots keep the un-bootstrapped return, so ``last_beam_values()`` stays the true returns while ``last_values()``
    and ``d_best_value`` carry the bootstrapped estimate of the best sequence and ``last_beam_keys()`` those of all kept ones.
    ``bootstrap="every"`` does so at every level, ``"last"`` at the last level only (the levels before it run as without a
    policy).  With ``width >= 3**horizon`` either equals the bootstrapped ``LookaheadPlanner(depth=horizon)`` bit for bit."""
    _handle_names = ("beam", "children")

    def __init__(self, root, width=9, horizon=32, gamma=1.0, substeps=None, value_policy=None, bootstrap="every"):
        self.bootstrap = check_bootstrap(bootstrap)
        check_value_policy(value_policy)
        self._attach(root, substeps)
        self.value_policy = check_value_policy(value_policy, self.root.device)
        self.weights = check_beam_args(self.n_roots, width, horizon, gamma)
        self.width, self.horizon, self.gamma = int(width), int(horizon), float(gamma)
        self.n_slots = self.n_roots * self.width
        self.n_children = 3 * self.n_slots
        self._open([("beam", self.n_slots), ("children", self.n_children)])

    def _build(self):
        ns, nc = self.n_slots, self.n_children
        self.d_root_map = self._dev(4 * ns, (np.arange(ns) // self.width).astype(np.int32))
        self.d_child_map = self._dev(4 * nc, (np.arange(nc) // 3).astype(np.int32))
        self.d_actions = self._dev(4 * nc, (np.arange(nc) % 3).astype(np.int32))
        self.d_slots = [self._dev(BEAM_SLOT.itemsize * ns), self._dev(BEAM_SLOT.itemsize * ns)]
        self.d_maps = self._dev(4 * ns * self.horizon)                      # int32[horizon][n_slots]
        self.d_best_value = self._dev(8 * self.n_roots)
        self.d_best_action = self._dev(4 * self.n_roots)
        views = self.children.device_views()
        self._d_reward = views["reward"].__cuda_array_interface__["data"][0]
        self._d_reason = views["reason"].__cuda_array_interface__["data"][0]
        if self.value_policy is not None:
            self._d_obs, self._obs_stride = views["obs"].__cuda_array_interface__["data"][0], views["stride"]
            self.d_leaf = self._dev(4 * nc)                                  # f32[n_children]: the value network at every child
            self.d_keys = self._dev(8 * ns)                                  # f64[n_slots]: what the last bootstrapped level ranked by
            boot = self.weights[-1] * self.gamma                             # w_H, the factor of the step after the last level
            if not np.isfinite(boot):
                raise ValueError("gamma**t overflows within the horizon")
            self.boot_weights = np.append(self.weights[1:], boot)            # level t's leaf counts with w_{t+1} = w_t * gamma

    def plan(self):
        """root -> every slot, then ``horizon`` levels of fork -> step -> select -> fork back, all enqueued on the root's stream
        (no copy, no synchronisation).  -> int32 (n_roots,) device view of the chosen actions, as ``LookaheadPlanner.plan()``."""
        lib = _lib.load()
        vp = C.c_void_p
        self.beam.fork_from(self.root, self.d_root_map.ptr)
        for t in range(self.horizon):
            self.children.fork_from(self.beam, self.d_child_map.ptr)
            self.children.step_device(self.d_actions.ptr, self.substeps)
            d_map = self.d_maps.ptr + 4 * self.n_slots * t
            d_in = vp(self.d_slots[(t + 1) % 2].ptr) if t else None
            if self.value_policy is not None and (self.bootstrap == "every" or t + 1 == self.horizon):
                self.value_policy.value_enqueue(self._d_obs, self._obs_stride, self.n_children, self.d_leaf.ptr, self.stream)
                check(lib.bsk_beam_select_boot(vp(self._d_reward), vp(self._d_reason), self.n_roots, self.width, t,
                                               float(self.weights[t]), float(self.boot_weights[t]), vp(self.d_leaf.ptr), d_in,
                                               vp(self.d_slots[t % 2].ptr), vp(d_map), vp(self.d_keys.ptr), vp(self.d_best_value.ptr),
                                               vp(self.d_best_action.ptr), vp(self.stream)))
            else:
                    check(lib.bsk_beam_select(vp(self._d_reward), vp(self._d_reason), self.n_roots, self.width, t, float(self.weights[t]),
                                          d_in, vp(self.d_slots[t % 2].ptr), vp(d_map), vp(self.d_best_value.ptr),
                                          vp(self.d_best_action.ptr), vp(self.stream)))
            if t + 1 < self.horizon:
                self.beam.fork_from(self.children, d_map)
        return self._actions_view()

    def _last_slots(self):
        return self._read(self.d_slots[(self.horizon - 1) % 2], BEAM_SLOT, self.n_slots)

    def last_beam_values(self):
        """discounted value of every kept sequence of the last plan, f64 (n_roots, width) in rank order (NaN: no sequence)"""
        return self._last_slots()["value"].reshape(self.n_roots, self.width)

    def last_beam_keys(self):
        """what the last level of the last plan ranked the kept sequences by, f64 (n_roots, width) in rank order: the value plus
        the discounted leaf value of the sequences still live (NaN: no sequence); needs a ``value_policy``"""
        if self.value_policy is None:
            raise ValueError("last_beam_keys: the planner has no value_policy")
        return self._read(self.d_keys, np.float64, self.n_slots).reshape(self.n_roots, self.width)

    def last_sequences(self):
        """the kept action sequences of the last plan, int32 (n_roots, width, horizon) in rank order, rebuilt from the level maps
        (the candidate c of a slot took action c % 3 from slot c // 3 of the level before).  A sequence whose episode ended
        continues with action 0; a slot without a sequence reads -1."""
        maps = self._read(self.d_maps, np.int32, self.n_slots * self.horizon).reshape(self.horizon, self.n_slots)
        seq = np.full((self.n_slots, self.horizon), -1, dtype=np.int32)
        c = maps[-1].astype(np.int64)
        for t in range(self.horizon - 1, -1, -1):
            ok = c >= 0
            seq[ok, t] = c[ok] % 3
            if t:
                c = np.where(ok, maps[t - 1][np.where(ok, c // 3, 0)], -1)
        return seq.reshape(self.n_roots, self.width, self.horizon)


def check_distill_args(n_steps, collect):
    """Argument rules of ``distill`` (no device needed) -> n_steps as an int."""
    if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or n_steps < 1:
        raise ValueError("n_steps must be an integer >= 1, got %r" % (n_steps,))
    if collect not in ("expert", "policy"):
        raise ValueError("collect must be 'expert' or 'policy', got %r" % (collect,))
    return int(n_steps)


def distill(planner, policy, fit, env, n_steps, collect="expert", value_targets=False):
    """Planner distillation (behaviour cloning) with no host in the loop: ``n_steps`` env steps of ``env`` - the
    ``BatchedPropagator`` (or an env over one) that is ``planner``'s root - and at each of them
      1. ``planner.plan()``, which leaves its labels in ``d_best_action`` and its values in ``d_best_value`` on the device;
      2. ``fit.accumulate`` on the root's own observation rows with those labels (and, with ``value_targets``, those values as the
         value network's targets) under the root's alive bytes (``bsk_fit_alive_mask``): every root counts at the first step - the
         observation it holds is labelled whatever its last step before the call left in the reason bytes, so reset a root whose
         episode is over before calling - and a root whose episode ends inside the loop contributes no more from the next step
         on, also when ``FLAG_AUTO_RESET`` starts it again;
      3. the root's step: on the planner's actions (``collect="expert"``), or on ``policy``'s own greedy actions for the same rows
         (``"policy"``: DAgger's collection rule - the states are the learner's, the labels the expert's);
      4. ``fit.step()``.
    ``fit`` is a ``PolicyFit`` attached to ``policy``.  Everything is enqueued on the root's stream: no copy to or from the host and
    no synchronisation until the loop has ended.  -> float64 (n_steps, 4), the diagnostics row of every step's accumulate
    (``policy_ref.FIT_STATS_COLUMNS``), read once at the end."""
    from . import _hip
    n_steps = check_distill_args(n_steps, collect)
    prop = getattr(env, "propagator", env)
    if planner.root is not prop:
        raise ValueError("the planner's root is not this env's propagator")
    if fit.policy is not policy:
        raise ValueError("the fit is attached to another policy")
    if value_targets and policy.spec.value_hidden is None:
        raise ValueError("value_targets: the policy has no value network")
    if policy.device != prop.device:
        raise ValueError("the policy lives on device %d, the propagator on device %d" % (policy.device, prop.device))
    lib, rt, vp = _lib.load(), _hip.runtime(), C.c_void_p
    n, stream = prop.n_envs, prop.stream_ptr()
    views = prop.device_views()
    obs, stride = views["obs"].__cuda_array_interface__["data"][0], views["stride"]
    reason = views["reason"].__cuda_array_interface__["data"][0]
    alive, rows = _hip.DeviceBuffer(n, prop.device), _hip.DeviceBuffer(32 * n_steps, prop.device)
    if collect == "policy":
        policy._buffers(n)                                 # (grown here, where a wait for the device is no wait inside the loop)
    try:
        with _hip.device_guard(prop.device):
            for t in range(n_steps):
                check(lib.bsk_fit_alive_mask(vp(reason), n, int(t == 0), vp(alive.ptr), vp(stream)))
                planner.plan()
                fit.accumulate(obs, planner.d_best_action.ptr, planner.d_best_value.ptr if value_targets else None, alive.ptr,
                               n=n, stride=stride, stream=stream)
                _hip.check(rt.hipMemcpyAsync(vp(rows.ptr + 32 * t), vp(fit.stats_ptr()), 32, _hip.hipMemcpyDeviceToDevice, vp(stream)),
                           "hipMemcpyAsync")
                actions = planner.d_best_action.ptr
                if collect == "policy":
                    actions = policy.enqueue(obs, stride, n, "greedy", (), getattr(prop, "env_base", 0), stream)["action"].ptr
                prop.step_device(actions, planner.substeps)
                fit.step(stream)
            out = np.empty((n_steps, 4), np.float64)
            _hip.check(rt.hipMemcpyAsync(vp(out.ctypes.data), vp(rows.ptr), out.nbytes, _hip.hipMemcpyDeviceToHost, vp(stream)),
                       "hipMemcpyAsync")
    finally:
        prop.sync()                                        # (the one wait: the rows are on the host, nothing queued reads the two buffers)
        alive.free()
        rows.free()
    return out


def demo(n=64, steps=40, depth=2, substeps=600, seed=0, beam=None):
    """A small batch of the full scenario (power system, Sun, drag, desaturation) run for ``steps`` env steps of ``substeps`` RK4
    steps under the planner and under each constant action, from the same initial conditions; prints the mean return per env
    (rewards summed until an env's episode ends).  ``beam``: (width, horizon) adds a ``BeamPlanner`` line.  Informative only: how
    the planners compare with constant actions is not a property the project asserts."""
    from ._lib import FLAG_DESAT, FLAG_DRAG, FLAG_POWER, FLAG_SUN_THIRD_BODY, GRAV_PM_J2
    from .simulators.dynamics import BatchedPropagator, default_config
    from .simulators.initial_conditions.batch import sample_ic_batch
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_POWER | FLAG_SUN_THIRD_BODY | FLAG_DRAG | FLAG_DESAT
    cfg.max_length = int(steps)
    ic = sample_ic_batch(n, 4, seed=seed)
    results = {}
    for policy in ("planner",) + (("beam",) if beam else ()) + (0, 1, 2):
        p = BatchedPropagator(cfg, n)
        p.reset(ic)
        planner = None
        if policy == "planner":
            planner = LookaheadPlanner(p, depth=depth, substeps=substeps)
        elif policy == "beam":
            planner = BeamPlanner(p, width=beam[0], horizon=beam[1], substeps=substeps)
        ret, live = np.zeros(n), np.ones(n, dtype=bool)
        for _ in range(int(steps)):
            act = planner.plan_host()[0] if planner else np.full(n, policy, np.int32)
            p.step(act, substeps)
            _, rew, done, _ = p.get_obs()
            ret += np.where(live, rew, 0.0)
            live &= ~done
            if not live.any():
                break
        results[policy] = float(ret.mean())
        if planner:
            planner.close()
        p.close()
    names = {"planner": "planner d=%d" % depth, "beam": "beam w=%d h=%d" % tuple(beam) if beam else ""}
    for policy, r in results.items():
        print("%-12s mean return %.6f" % (names.get(policy, "action %s" % policy), r))
    return results


if __name__ == "__main__":
    import sys
    demo(beam=(9, 32) if "--beam" in sys.argv[1:] else None)
