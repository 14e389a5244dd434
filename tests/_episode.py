"""Teacher-forced parity along whole episodes, for tests (tests/test_episode_host.py, tests/test_gpu_episode.py).

The device (a ``BatchedPropagator``, or tests/_oracle_backend.py's stand-in) runs an episode freely under a scripted host policy.
Before every env step the oracle is restarted from the device's OWN state and counters, so an env step's error is that of one
launch from the state the device is in - errors do not accumulate, and the one-call bounds of tests/test_gpu_bench_shapes.py for a
full-scenario launch of 1 800 sub-steps apply at every step, as late in the episode as it gets (``BOUNDS``).

An env step counts while its spacecraft was not done BEFORE the step: the terminating step counts, nothing after it (the vec env
would have restarted the spacecraft).  The episode stops early once every spacecraft is done.

A step from a late state can be ill conditioned (a wheel about to run away, a value on a dead-band).  That is MEASURED, not
allowed for: for every env step over a numeric bound the oracle runs again from the same saved input with every continuous state
value moved by a seeded random +/- 2^-52 relative amount (``twin_input``).  Only if this twin moves a state group by more than
``TWIN_LIMIT`` (ten times the worst twin movement over a step from a fresh initial condition, 1.2e-13 - the regime the bounds were
set in) is the env step excused from the numeric bounds; reason, done and counters stay exact for it.  Everything else over a
bound is a ``failures`` entry.  Nothing here asserts: the tests do, on what ``run_episode`` returns.
"""
import time

import numpy as np

from helpers import field_groups
from oracle import oracle

BOUNDS = {"state": 1e-10, "obs": 1e-9, "reward": 1e-12, "charge": 1e-7}
TWIN_LIMIT = 1e-12
EXCUSED_CAP = 0.002        # of an episode's env steps


# ------------------------------------------------------------------------------------------------------------------ policies
class Keeper(object):
    """Point (0); charge (1) where the battery is under 0.35; desaturate (2) where the wheels are over half their limit."""
    name = "keeper"

    def __call__(self, t, obs, n):
        a = np.zeros(n, np.int32)
        if obs is not None:
            a[obs[3] < 0.35] = 1
            a[obs[2] > 0.5] = 2
        return a


class Random(object):
    name = "random"

    def __init__(self, seed=1):
        self.rng = np.random.default_rng(seed)

    def __call__(self, t, obs, n):
        return self.rng.integers(0, 3, n).astype(np.int32)


class Nadir(object):
    name = "nadir"

    def __call__(self, t, obs, n):
        return np.zeros(n, np.int32)


POLICIES = {"keeper": Keeper, "random": Random, "nadir": Nadir}


# ------------------------------------------------------------------------------------------------------------------ errors
def group_err_per_env(a, b, n_rw):
    """helpers.max_group_err per env: {group: (n,) max |a - b| over the group's rows, relative to the group's largest magnitude in
    the whole batch ``b``}."""
    return {k: np.abs(a[sl] - b[sl]).max(axis=0) / max(np.abs(b[sl]).max(), 1e-300) for k, sl in field_groups(n_rw).items()}


def _worst_group(errs):
    """(n,) largest group error per env (NaN where any group's is NaN), (n,) name of that group"""
    names = list(errs)
    m = np.stack([errs[k] for k in names])
    bad = np.isnan(m).any(axis=0)
    arg = np.where(bad, 0, np.nanargmax(np.where(np.isnan(m), -1.0, m), axis=0))
    return np.where(bad, np.nan, m[arg, np.arange(m.shape[1])]), np.array(names)[arg]


def continuous_rows(n_rw):
    """Rows of the slab that hold continuous dynamic values: r, v, sigma, omega, wheel speeds, the held and the pending wheel torque,
    the battery charge and the thrusters' owed on-times.  (Not the disturbance torque, a constant of the episode; not the burst
    limits, burst start tick and dumping counter, which are integers; not the |sigma_BR| message, which the dynamics do not read.)"""
    t = 12 + n_rw
    return np.r_[0:t, t + 3:t + 3 + n_rw, t + 7, t + 8:t + 16, t + 26:t + 26 + n_rw]


def twin_input(state, n_rw, rng):
    """A copy of ``state`` with every continuous value moved by +/- 2^-52 of itself."""
    tw = state.copy()
    rows = continuous_rows(n_rw)
    tw[rows] *= 1.0 + rng.choice([-1.0, 1.0], size=(rows.size, state.shape[1])) * 2.0 ** -52
    return tw


def _oracle_step(cfg, st, steps, ticks, a, k):
    st, steps, ticks = np.ascontiguousarray(st), steps.copy(), ticks.copy()
    out = oracle.step(cfg, st, steps, ticks, np.ascontiguousarray(a, np.int32), k, omp=True)
    return st, steps, ticks, out


# ------------------------------------------------------------------------------------------------------------------ harness
def run_episode(device, cfg, ic, policy, T=541, k=1800, twin="over", twin_seed=0):
    """Reset ``device`` to ``ic`` and run up to ``T`` env steps of ``k`` sub-steps under ``policy`` (``policy(t, obs, n)`` ->
    int32 actions; ``obs`` is the device's observation, None before the first step).

    ``twin``: "over" runs the perturbed twin for the env steps over a numeric bound only, "all" for every env step (the share
    of ill-conditioned steps of the episode, ``twin_over`` / ``env_steps``).

    Returns a dict:
      env_steps              env steps compared
      err                    {"state", "obs", "reward", "charge"}: (T, n) error per env step, NaN where not compared
      worst                  the same four: the largest error among the env steps that were not excused
      worst_group            the state group of worst["state"], its step and env
      excused                [{step, env, action, wheel_fraction, charge_fraction, shadow, err: {...}, twin}]
      failures               [{step, env, what, ...}]: unexcused env steps over a bound; ANY difference in reason, done or counters
      twin_over, twin_max    env steps whose twin moved a state group by more than TWIN_LIMIT (of those it ran for); its largest movement
      twin_flipped_reason    env steps whose twin ended with another reason
      regimes                counters over the compared env steps (see the code)
      end_step, end_reason   per spacecraft: the step at which it was done (T where never), the reason word of that step
      t_device, t_oracle     seconds spent stepping and reading the device / in the oracle
    """
    n, n_rw = ic.shape[1], int(cfg.n_rw)
    cap = float(cfg.storage_capacity)
    charge_row = 12 + n_rw + 7
    rng = np.random.default_rng(twin_seed)
    device.reset(ic)
    live = np.ones(n, bool)
    err = {key: np.full((T, n), np.nan) for key in BOUNDS}
    worst = {key: 0.0 for key in BOUNDS}
    res = {"env_steps": 0, "err": err, "worst": worst, "worst_group": None, "excused": [], "failures": [], "twin_over": 0,
           "twin_max": 0.0, "twin_flipped_reason": 0, "end_step": np.full(n, T), "end_reason": np.zeros(n, np.uint8),
           "t_device": 0.0, "t_oracle": 0.0}
    reg = {"full_battery": 0, "penumbra": 0, "umbra": 0, "sunlit": 0, "max_wheel_fraction_live": 0.0, "min_sigma_BR": np.inf,
           "min_charge_fraction": np.inf, "actions": np.zeros(3, np.int64), "max_ticks": 0, "steps_run": 0}
    res["regimes"] = reg
    obs = None
    for t in range(T):
        if not live.any():
            break
        idx = np.flatnonzero(live)
        a = np.asarray(policy(t, obs, n), np.int32)
        c0 = time.perf_counter()
        st0 = device.get_state()
        steps0, ticks0 = device.get_counters()
        device.step(a, k)
        got = device.get_obs()
        st1 = device.get_state()
        steps1, ticks1 = device.get_counters()
        c1 = time.perf_counter()
        obs, rew, done, why = (np.asarray(x) for x in got)
        # the oracle from the device's own input, live spacecraft only
        o_st, o_steps, o_ticks, (o_obs, o_rew, o_done, o_why) = _oracle_step(cfg, st0[:, idx], steps0[idx], ticks0[idx], a[idx], k)
        g_st = st1[:, idx]
        gerr, gname = _worst_group(group_err_per_env(g_st, o_st, n_rw))
        e = {"state": gerr, "obs": np.abs(obs[:, idx] - o_obs).max(axis=0), "reward": np.abs(rew[idx] - o_rew),
             "charge": np.abs(g_st[charge_row] - o_st[charge_row]) / cap}
        over = np.zeros(idx.size, bool)
        for key, bound in BOUNDS.items():
            err[key][t, idx] = e[key]
            over |= ~(e[key] <= bound)                                 # (NaN is over)
        exact = {"reason": np.asarray(why)[idx].astype(np.int64) != o_why.astype(np.int64),
                 "done": np.asarray(done)[idx].astype(bool) != o_done.astype(bool),
                 "steps": steps1[idx] != o_steps, "ticks": ticks1[idx] != o_ticks}
        for what, bad in exact.items():
            res["failures"] += [{"step": t, "env": int(idx[j]), "what": what, "action": int(a[idx[j]])} for j in np.flatnonzero(bad)]
        # the twin: where a numeric bound is passed, or everywhere
        tw = np.flatnonzero(over) if twin == "over" else np.arange(idx.size)
        moved = np.zeros(idx.size)
        if tw.size:
            w_st, _, _, w_out = _oracle_step(cfg, twin_input(st0[:, idx[tw]], n_rw, rng), steps0[idx[tw]], ticks0[idx[tw]], a[idx[tw]], k)
            scale = {key: max(np.abs(o_st[sl]).max(), 1e-300) for key, sl in field_groups(n_rw).items()}
            moved[tw] = np.max([np.abs(w_st[sl] - o_st[sl][:, tw]).max(axis=0) / scale[key] for key, sl in field_groups(n_rw).items()], axis=0)
            res["twin_over"] += int((~(moved[tw] <= TWIN_LIMIT)).sum())
            res["twin_max"] = max(res["twin_max"], float(np.nanmax(moved[tw])))
            res["twin_flipped_reason"] += int((w_out[3] != o_why[tw]).sum())
        c2 = time.perf_counter()
        res["t_device"] += c1 - c0
        res["t_oracle"] += c2 - c1
        for j in np.flatnonzero(over):
            rec = {"step": t, "env": int(idx[j]), "action": int(a[idx[j]]), "wheel_fraction": float(obs[2, idx[j]]),
                   "charge_fraction": float(obs[3, idx[j]]), "shadow": float(obs[4, idx[j]]), "group": str(gname[j]),
                   "err": {key: float(e[key][j]) for key in BOUNDS}, "twin": float(moved[j])}
            if moved[j] > TWIN_LIMIT:
                res["excused"].append(rec)
            else:
                res["failures"].append(dict(rec, what=[key for key in BOUNDS if not e[key][j] <= BOUNDS[key]]))
        for key in BOUNDS:
            ok = e[key][~over]
            if ok.size and ok.max() > worst[key]:
                worst[key] = float(ok.max())
                if key == "state":
                    j = np.flatnonzero(~over)[np.argmax(ok)]
                    res["worst_group"] = (str(gname[j]), t, int(idx[j]))
        # regimes, on the device's values of the compared env steps
        res["env_steps"] += idx.size
        reg["steps_run"] = t + 1
        reg["full_battery"] += int((g_st[charge_row] == cap).sum())
        sh = obs[4, idx]
        reg["penumbra"] += int(((sh > 0.0) & (sh < 1.0)).sum())
        reg["umbra"] += int((sh == 0.0).sum())
        reg["sunlit"] += int((sh == 1.0).sum())
        reg["actions"] += np.bincount(a[idx], minlength=3)[:3]
        reg["max_ticks"] = max(reg["max_ticks"], int(ticks1[idx].max()))
        ended = np.asarray(done)[idx].astype(bool)
        res["end_step"][idx[ended]] = t + 1
        res["end_reason"][idx[ended]] = np.asarray(why)[idx][ended]
        live[idx[ended]] = False
        if live.any():                                                 # spacecraft that go on: where the next step starts from
            reg["max_wheel_fraction_live"] = max(reg["max_wheel_fraction_live"], float(obs[2, live].max()))
            reg["min_sigma_BR"] = min(reg["min_sigma_BR"], float(obs[0, live].min()))
            reg["min_charge_fraction"] = min(reg["min_charge_fraction"], float(obs[3, live].min()))
    return res


def report(tag, res):
    """The lines a test prints for one episode (pytest -s)."""
    reg = res["regimes"]
    n_ex = len(res["excused"])
    lines = ["[episode %s] %d env steps compared in %d steps; device %.2f s, oracle %.2f s"
             % (tag, res["env_steps"], reg["steps_run"], res["t_device"], res["t_oracle"]),
             "  worst unexcused error: " + ", ".join("%s %.3g (bound %.0e)" % (key, res["worst"][key], BOUNDS[key]) for key in BOUNDS)
             + "; state group " + str(res["worst_group"]),
             "  excused %d = %.4f %% (cap %.1f %%); failures %d; twin over %.0e on %d env steps, largest %.3g, reason flips %d"
             % (n_ex, 100.0 * n_ex / max(res["env_steps"], 1), 100.0 * EXCUSED_CAP, len(res["failures"]), TWIN_LIMIT, res["twin_over"],
                res["twin_max"], res["twin_flipped_reason"])]
    lines += ["    excused " + str(rec) for rec in res["excused"]]
    lines += ["    FAILURE " + str(rec) for rec in res["failures"][:40]]
    ends = {int(w): int((res["end_reason"] == w).sum()) for w in np.unique(res["end_reason"])}
    lines.append("  regimes: ended by reason word %s, %d at the last step; full battery %d, penumbra %d, umbra %d, sunlit %d; max live wheel "
                 "fraction %.3f, min |sigma_BR| %.3g, min charge fraction %.3f; actions %s; max tick counter %d"
                 % (ends, int((res["end_step"] == reg["steps_run"]).sum()), reg["full_battery"], reg["penumbra"], reg["umbra"], reg["sunlit"],
                    reg["max_wheel_fraction_live"], reg["min_sigma_BR"], reg["min_charge_fraction"], reg["actions"].tolist(), reg["max_ticks"]))
    return "\n".join(lines)


def check(res):
    """What every teacher-forced episode must satisfy; returns nothing, raises AssertionError with the offending env steps."""
    assert not res["failures"], res["failures"][:10]
    assert len(res["excused"]) <= EXCUSED_CAP * res["env_steps"], res["excused"]
