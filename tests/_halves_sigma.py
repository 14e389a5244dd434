"""The batches of tests/test_gpu_halves_sigma.py and the proof that they hold what that file claims (tests/test_halves_sigma_host.py).
CPU only: nothing here runs a kernel.

The halves form's rotational wave integrates the angular velocity in front of the hand-over and the attitude behind the form's last
barrier, from the four stage angular velocities it kept (csrc/bsk_device.hpp: rk4_rot_omega, rk4_rot_sigma).  What that can break is
the attitude alone: a stage rate taken from the wrong stage, the shadow-set switch in some lanes of a wave and not in others, the
deferred stores of tail lanes.  So the batches are the characters of tests/_crowd.py whose attitude moves most:

  wave 0           mixed: 16 `cross` (|sigma| close to 1 with 0.1 rad/s along sigma: the switch falls inside the schedule for about half
                   of them, later for the rest), 16 `spin` (wheel speeds x 2.5: the gyroscopic term makes the four
                   stage rates differ in many bits), 16 `mid_a` (ticks 1 .. 16: every FSW phase, so every launch is the one before, at
                   and after an FSW tick of some lane), 8 `mid_b`, 8 `mid_c` - round-robin, so that neighbours differ
  n = 65           env 64: a `cross` character that switches; the 63 other lanes of its wave shadow it
  n = 130          wave 1: `cross` characters that switch, repeated to fill the wave - every lane crosses; envs 128, 129: one that
                   switches and a `spin`, shadowed by 62 lanes

SCHEDULE  25 launches of one sub-step, random per-env actions: two FSW ticks of every lane fall inside.  "Switches" is decided by the
oracle: sigma before and after a launch point away from each other and |sigma| was above 0.9 (the test of _crowd.prove)."""
import numpy as np

import _crowd as C
import test_gpu_kernel_info as KI
from basilisk_env_amd._lib import GRAV_PM, GRAV_PM_J2
from oracle import oracle

LAUNCHES = 25
SIZES = (65, 130)
CELLS = [(GRAV_PM_J2, 4, True), (GRAV_PM, 3, False)]       # 4 and 3 wheels, diagonal and general hub
_BUILT = {}


def run_oracle(cfg, state, steps, ticks, actions):
    """The schedule on the oracle -> per launch (state, obs, reward, done, reason, steps, ticks), copies; env on the last axis"""
    st, steps, ticks = np.array(state, dtype=np.float64, order="C"), steps.copy(), ticks.copy()
    out = []
    for act in actions:
        obs, rew, done, why = oracle.step(cfg, st, steps, ticks, np.ascontiguousarray(act, np.int32), 1)
        out.append((st.copy(), obs.copy(), rew.copy(), done.copy(), why.copy(), steps.copy(), ticks.copy()))
    return out


def switches(state, runs):
    """-> (launches, n) bool: the shadow-set switch of env e falls inside launch t"""
    sig = [state[6:9]] + [r[0][6:9] for r in runs]
    return np.array([((a * b).sum(axis=0) < 0.0) & ((a * a).sum(axis=0) > 0.81) for a, b in zip(sig[:-1], sig[1:])])


class Batch(object):
    """cfg; state (n_fields, n), steps, ticks (n,): what each env starts from; actions (LAUNCHES, n); slot (n,) names; ref: the
    oracle's run of the schedule; switched (LAUNCHES, n)"""

    def __init__(self, cfg, cast, crossing, n):
        pick = lambda name, k: list(cast.where(name)[:k])       # noqa: E731
        groups = [pick("cross", 16), pick("spin", 16), pick("mid_a", 16), pick("mid_b", 8) + pick("mid_c", 8)]
        index = [g[k] for k in range(16) for g in groups]       # round-robin: cross, spin, mid_a, mid_b / mid_c, cross, ...
        if n == 65:
            index += [crossing[0]]
        else:
            index += [crossing[k % len(crossing)] for k in range(64)] + [crossing[-1], pick("spin", 1)[0]]
        assert len(index) == n
        self.cfg, self.n, self.index = cfg, n, np.array(index)
        self.slot = cast.slot[self.index]
        self.state = np.ascontiguousarray(cast.state[:, self.index])
        self.steps, self.ticks = cast.steps[self.index].copy(), cast.ticks[self.index].copy()
        self.actions = np.random.default_rng([n, cfg.n_rw]).integers(0, 3, (LAUNCHES, n)).astype(np.int32)
        self.ref = run_oracle(cfg, self.state, self.steps, self.ticks, self.actions)
        self.switched = switches(self.state, self.ref)


def batch(grav, n_rw, diag, n):
    """The batch of one cell and size (built once per process: the tests that share it leave it unchanged)"""
    key = (grav, n_rw, diag)
    if key not in _BUILT:
        cfg = C.crowd_config(KI.config(grav, n_rw, "bare", diag), "bare")
        cast = C.Cast(cfg, "bare")
        mine = cast.where("cross")
        acts = np.random.default_rng([7, n_rw]).integers(0, 3, (LAUNCHES, mine.size)).astype(np.int32)
        st = np.ascontiguousarray(cast.state[:, mine])
        # (a character's switch depends on its actions only through the wheel torques: decided again, under the batch's own
        # actions, by ``Batch.switched`` - test_halves_sigma_host.py holds the two to the same answer)
        crossing = mine[switches(st, run_oracle(cfg, st, cast.steps[mine], cast.ticks[mine], acts)).any(axis=0)]
        assert crossing.size >= 4, crossing
        _BUILT[key] = (cfg, cast, list(crossing), {})
    cfg, cast, crossing, sized = _BUILT[key]
    if n not in sized:
        sized[n] = Batch(cfg, cast, crossing, n)
    return sized[n]
