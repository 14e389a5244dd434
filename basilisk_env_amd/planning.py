"""Batched lookahead planning on the GPU: "plan, then act" for thousands of spacecraft without a host visit.

``LookaheadPlanner`` forks every root env into ``3**depth`` branches (``bsk_fork_device``), rolls every branch out under its own
action sequence for ``depth + tail_steps`` env steps (``bsk_step_n``) and picks, per root, the first action of the branch with the
greatest discounted return (``bsk_select_branches``).  Branch b takes base-3 digit t of b at step t < depth, then ``tail_action``;
the branch's return stops after the first step that ends its episode (that step's reward and penalty included).  All three are
enqueued on the root's stream from buffers built once, so ``plan()`` - and a step of the root on the planned actions - can be
captured into one HIP graph.  An extra beside the reference surface: the reference has no forking or planning.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import FLAG_AUTO_RESET, FLAG_EPISODE_STATS, FLAG_LDS_SCRATCH, FLAG_OBS_ROWMAJOR, GRAV_SH, check

MAX_DEPTH = 6
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


class LookaheadPlanner(object):
    """Exhaustive lookahead of ``depth`` env steps (3**depth branches per root), then ``tail_steps`` steps of ``tail_action``.

    ``root``: a ``BatchedPropagator`` (``substeps`` required) or a ``LeoPowerAttVecEnv`` (its ``propagator`` and ``substeps``).
    The planner owns a branch propagator of ``n_roots * 3**depth`` envs on the root's device and stream with the root's config
    minus ``BRANCH_CLEARED_FLAGS``, the root's sim time and spherical-harmonic field, and device buffers built once: the fork map,
    the action table, the histories and the outputs.  A later ``set_sim_time`` / ``set_gravity_sh`` on the root needs a new planner
    (the fork refuses partners that differ)."""

    def __init__(self, root, depth=2, tail_steps=0, tail_action=0, gamma=1.0, substeps=None):
        from .simulators.dynamics import BatchedPropagator
        prop = getattr(root, "propagator", root)
        if substeps is None:
            substeps = getattr(root, "substeps", None)
        if not isinstance(prop, BatchedPropagator):
            raise TypeError("LookaheadPlanner needs a BatchedPropagator or a LeoPowerAttVecEnv over one (sharded propagators are not "
                            "supported: fork within each shard)")
        if substeps is None or int(substeps) < 1:
            raise ValueError("substeps (RK4 steps per env step) is required for a BatchedPropagator root")
        self.n_roots = int(prop.n_envs)
        self.n_branch = check_args(self.n_roots, depth, tail_steps, tail_action, gamma)
        self.depth, self.tail_steps, self.tail_action, self.gamma = int(depth), int(tail_steps), int(tail_action), float(gamma)
        self.group = 3 ** self.depth
        self.n_steps = self.depth + self.tail_steps
        self.substeps = int(substeps)
        self.root = prop
        if prop.cfg.gravity_model == GRAV_SH and prop.gravity_sh is None:
            raise ValueError("the root has no spherical-harmonic field yet (set_gravity_sh)")
        self._buffers = []
        cfg = prop.cfg.copy()
        cfg.flags &= ~BRANCH_CLEARED_FLAGS
        self.stream = prop.stream_ptr()
        self.branch = BatchedPropagator(cfg, self.n_branch, device=prop.device, stream=self.stream)
        try:
            if prop.sim_time:
                self.branch.set_sim_time(prop.sim_time)
            if prop.gravity_sh is not None:
                self.branch.set_gravity_sh(*prop.gravity_sh)
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

    def plan(self):
        """fork -> ``depth + tail_steps`` env steps of every branch -> per-root choice, all enqueued on the root's stream (no copy,
        no synchronisation).  -> int32 (n_roots,) device view of the chosen actions (``__cuda_array_interface__`` / DLPack):
        ``root.step_device(view.__cuda_array_interface__["data"][0], ...)`` and ``torch.from_dlpack(view)`` take it as it is."""
        from .simulators.dynamics.propagator import _DevArray
        self.branch.fork_from(self.root, self.d_map.ptr)
        self.branch.step_n(self.n_steps, self.substeps, self.d_actions.ptr, d_reward_hist=self.d_reward_hist.ptr,
                           d_reason_hist=self.d_reason_hist.ptr)
        check(_lib.load().bsk_select_branches(C.c_void_p(self.d_reward_hist.ptr), C.c_void_p(self.d_reason_hist.ptr),
                                              C.c_void_p(self.d_first_action.ptr), self.n_steps, self.n_branch, self.group, self.gamma,
                                              C.c_void_p(self.d_values.ptr), C.c_void_p(self.d_best_value.ptr),
                                              C.c_void_p(self.d_best_action.ptr), C.c_void_p(self.stream)))
        return _DevArray(self.d_best_action.ptr, (self.n_roots,), "<i4", owner=self.root, device=self.root.device, stream=self.stream)

    def _read(self, buf, dtype, count):
        from . import _hip
        out = np.empty(count, dtype=dtype)
        _hip.check(_hip.runtime().hipMemcpyAsync(C.c_void_p(out.ctypes.data), C.c_void_p(buf.ptr), out.nbytes, _hip.hipMemcpyDeviceToHost,
                                                 C.c_void_p(self.stream)), "hipMemcpyAsync")
        self.root.sync()
        self.branch.sync()           # (reports a fork's device error, if any)
        return out

    def plan_host(self):
        """``plan()``, then -> (actions int32 (n_roots,), values f64 (n_roots,)) on the host (synchronises)."""
        self.plan()
        return self.last_actions(), self.last_values()

    def last_actions(self):
        return self._read(self.d_best_action, np.int32, self.n_roots)

    def last_values(self):
        """best branch value per root of the last plan"""
        return self._read(self.d_best_value, np.float64, self.n_roots)

    def last_branch_values(self):
        """value of every branch of the last plan, f64 (n_roots, 3**depth)"""
        return self._read(self.d_values, np.float64, self.n_branch).reshape(self.n_roots, self.group)

    def close(self):
        if getattr(self, "branch", None) is not None:
            self.branch.sync()
            self.branch.close()
            self.branch = None
        for b in getattr(self, "_buffers", []):
            b.free()
        self._buffers = []


def demo(n=64, steps=40, depth=2, substeps=600, seed=0):
    """A small batch of the full scenario (power system, Sun, drag, desaturation) run for ``steps`` env steps of ``substeps`` RK4
    steps under the planner and under each constant action, from the same initial conditions; prints the mean return per env
    (rewards summed until an env's episode ends).  Informative only: how the planner compares with constant actions is not a
    property the project asserts."""
    from ._lib import FLAG_DESAT, FLAG_DRAG, FLAG_POWER, FLAG_SUN_THIRD_BODY, GRAV_PM_J2
    from .simulators.dynamics import BatchedPropagator, default_config
    from .simulators.initial_conditions.batch import sample_ic_batch
    cfg = default_config(4, GRAV_PM_J2)
    cfg.flags |= FLAG_POWER | FLAG_SUN_THIRD_BODY | FLAG_DRAG | FLAG_DESAT
    cfg.max_length = int(steps)
    ic = sample_ic_batch(n, 4, seed=seed)
    results = {}
    for policy in ("planner", 0, 1, 2):
        p = BatchedPropagator(cfg, n)
        p.reset(ic)
        planner = LookaheadPlanner(p, depth=depth, substeps=substeps) if policy == "planner" else None
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
    for policy, r in results.items():
        print("%-12s mean return %.6f" % ("planner d=%d" % depth if policy == "planner" else "action %d" % policy, r))
    return results


if __name__ == "__main__":
    demo()
