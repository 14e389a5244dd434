"""The scenario of the episode-outcome tests (tests/test_gpu_outcomes.py): envs staggered so that, inside a rollout of a dozen env
steps, episodes end for different reasons and at different steps while others never end, under one policy per member that uses more
than one action.  Written against the interface ``BatchedPropagator`` and tests/_oracle_backend.py share, so that what the
staggering produces can be looked at on the CPU oracle as well.  TEST CODE."""
import numpy as np

from _policy_bounds import centred, reset_observations, seeded_policy
from basilisk_env_amd import _lib
from basilisk_env_amd import policy_ref as R
from basilisk_env_amd._lib import DONE_BATTERY, DONE_LENGTH, DONE_WHEELS, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch

N_RW, MAX_LENGTH = 4, 40


def config(flags=0, max_length=MAX_LENGTH):
    cfg = default_config(N_RW, GRAV_PM_J2)
    cfg.flags |= flags
    cfg.max_length = max_length
    return cfg


def members(n_members, hidden=(16,), seed=0, value_hidden=None):
    """-> (Spec, params (P, n_params)): a seeded relu network per member (with ``value_hidden`` a value network as well: the sixth
    history of a rollout), its output biases centred on reset observations so that all three actions occur"""
    blocks = []
    for m in range(n_members):
        spec, block = seeded_policy(hidden, "relu", value_hidden, seed=seed + 17 * m)
        blocks.append(centred(spec, block, reset_observations(sample_ic_batch(500, N_RW, seed=m), default_config(N_RW, GRAV_PM_J2))))
    return spec, np.stack(blocks)


def stagger(prop, cfg):
    """By env index i mod 8, on a handle that has been reset and stepped once:
         1  no charge: BATTERY at the rollout's first step (dead at step 0);
         2  wheel speeds scaled to 1.02 (every other one: 0.9999) of the limit: WHEELS at the first step, or whenever the wheels
            next speed up;
         3  the step counter (i // 8) mod 10 short of max_length: LENGTH at that step of the rollout;
       everything else is left to run: unfinished when a rollout shorter than max_length ends."""
    state = prop.get_state()
    steps, ticks = prop.get_counters()
    n = state.shape[1]
    i = np.arange(n)
    tail = _lib.NF_BASE + N_RW
    state[tail + _lib.T_CHARGE, i % 8 == 1] = 0.0
    fast = i % 8 == 2
    om = state[_lib.NF_BASE:tail, fast]
    frac = np.where((i[fast] // 8) % 2 == 0, 1.02, 0.9999)
    state[_lib.NF_BASE:tail, fast] = om / np.linalg.norm(om, axis=0) * cfg.wheel_limit * frac
    late = i % 8 == 3
    steps[late] = cfg.max_length - (i[late] // 8) % 10
    prop.set_state(state)
    prop.set_counters(steps, ticks)


def what_happened(reason_hist, action_hist):
    """What the recorded histories (T, n) hold of what the scenario is for -> dict of counts over the FIRST episodes"""
    q, a = np.asarray(reason_hist), np.asarray(action_hist)
    T, n = q.shape
    ended = (q != 0).any(axis=0)
    first = np.where(ended, (q != 0).argmax(axis=0), T - 1)
    end = np.where(ended, q[first, np.arange(n)], 0)
    alive = np.arange(T)[:, None] <= first[None, :]
    return {"length": int(((end & DONE_LENGTH) != 0).sum()), "wheels": int(((end & DONE_WHEELS) != 0).sum()),
            "battery": int(((end & DONE_BATTERY) != 0).sum()), "unfinished": int((~ended).sum()),
            "actions": sorted(set(a[alive].tolist())), "end_steps": sorted(set(first[ended].tolist())),
            "later_ends": int(((q != 0) & ~alive).sum())}


def assert_not_vacuous(reason_hist, action_hist):
    w = what_happened(reason_hist, action_hist)
    assert w["length"] >= 1 and w["wheels"] + w["battery"] >= 1 and w["unfinished"] >= 1 and len(w["actions"]) >= 2, w
    assert len(w["end_steps"]) >= 3, w                     # (the endings are staggered over the rollout)
    return w


def oracle_histories(prop, spec, params, T, k, E):
    """The closed loop on a propagator with host results (tests/_oracle_backend.py), greedy: member j // E of ``params`` chooses the
    action of env j from the current observation, by the numpy chain -> (reward, reason, action) histories (T, n)"""
    n = prop.n_envs
    reward, reason, action = np.empty((T, n)), np.empty((T, n), np.uint8), np.empty((T, n), np.int32)
    for t in range(T):
        obs = prop.get_obs()[0]
        for m in range(n // E):
            cols = slice(m * E, (m + 1) * E)
            logits, _ = R.mlp_ref(spec, params[m], obs[:, cols])
            action[t, cols] = R.act_ref(logits, "greedy")[0]
        prop.step(action[t], k)
        _, reward[t], _, reason[t] = prop.get_obs()
    return reward, reason, action
