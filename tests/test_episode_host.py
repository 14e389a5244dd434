"""CPU: the whole-episode harness of tests/_episode.py on itself, with tests/_oracle_backend.py's stand-in as the device.

Eight spacecraft of the full scenario fly the reference episode (541 env steps of 1 800 sub-steps) under the keeper policy:
- the stand-in IS the oracle, so every error is exactly 0, nothing is excused and nothing fails;
- the perturbed twin runs for EVERY env step: the share of steps it moves by more than ``TWIN_LIMIT`` - the ill-conditioned ones,
  the only ones the GPU tests may excuse - stays under the cap the GPU tests allow, and it flips no reason;
- a stand-in whose state is corrupted once, after step 300 (one wheel speed scaled by 1 + 1e-9: host arrays only), is reported as
  ONE unexcused failure, at that step, for that spacecraft, in the wheel-speed group - and nowhere else, since the oracle restarts
  from the stand-in's state at the next step."""
import numpy as np
import pytest

import _episode
from _oracle_backend import OmpOraclePropagator
from basilisk_env_amd._lib import FLAG_DESAT, FLAG_DRAG, FLAG_POWER, FLAG_SUN_THIRD_BODY, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch

N, N_RW = 8, 4


def _cfg():
    cfg = default_config(N_RW, GRAV_PM_J2)
    cfg.flags |= FLAG_POWER | FLAG_SUN_THIRD_BODY | FLAG_DRAG | FLAG_DESAT
    return cfg


@pytest.fixture(scope="module")
def clean():
    cfg = _cfg()
    res = _episode.run_episode(OmpOraclePropagator(cfg, N), cfg, sample_ic_batch(N, N_RW, seed=5), _episode.Keeper(), twin="all")
    print(_episode.report("host keeper n=8", res))
    return res


def test_stand_in_has_zero_error_along_the_whole_episode(clean):
    _episode.check(clean)
    assert clean["env_steps"] > 3000 and clean["regimes"]["steps_run"] == 541
    assert clean["regimes"]["max_ticks"] == 541 * 1800
    assert not clean["excused"] and not clean["failures"]
    for key in _episode.BOUNDS:
        e = clean["err"][key]
        assert int(np.isfinite(e).sum()) == clean["env_steps"] and np.nanmax(e) == 0.0, key
    assert clean["worst"] == {key: 0.0 for key in _episode.BOUNDS}


def test_twin_share_stays_under_the_cap(clean):
    """The twin ran for every env step: the steps it moves by more than TWIN_LIMIT are the ones the GPU tests would excuse if the
    device missed a bound there."""
    assert clean["twin_max"] > 0.0                                     # it does perturb
    assert clean["twin_over"] <= _episode.EXCUSED_CAP * clean["env_steps"], (clean["twin_over"], clean["env_steps"], clean["twin_max"])
    assert clean["twin_flipped_reason"] == 0


class _Corrupted(OmpOraclePropagator):
    """Scales the largest wheel speed among the spacecraft ``envs`` by 1 + 1e-9 in the state that step ``at`` (0-based) leaves."""

    def __init__(self, cfg, n, at, envs):
        super().__init__(cfg, n)
        self.at, self.envs, self.calls, self.env = at, np.asarray(envs), 0, None

    def step(self, actions, substeps):
        super().step(actions, substeps)
        if self.calls == self.at:
            om = self.state[12:12 + self.n_rw]
            w, j = np.unravel_index(np.argmax(np.abs(om[:, self.envs])), (self.n_rw, self.envs.size))
            self.env = int(self.envs[j])
            om[w, self.env] *= 1.0 + 1e-9
        self.calls += 1


def test_corrupted_stand_in_is_reported_at_its_step_and_env(clean):
    cfg = _cfg()
    dev = _Corrupted(cfg, N, 300, np.flatnonzero(clean["end_step"] > 302))    # the spacecraft still flying then
    res = _episode.run_episode(dev, cfg, sample_ic_batch(N, N_RW, seed=5), _episode.Keeper(), T=303)
    env = dev.env
    # 1e-9 of the largest wheel speed of the compared batch: ten times the bound on a state group
    assert [(f["step"], f["env"], f["what"], f["group"]) for f in res["failures"]] == [(300, env, ["state"], "Omega")], res["failures"]
    assert res["failures"][0]["twin"] <= _episode.TWIN_LIMIT and not res["excused"]
    assert abs(res["failures"][0]["err"]["state"] / 1e-9 - 1.0) < 1e-3
    with pytest.raises(AssertionError):
        _episode.check(res)
    e = res["err"]["state"].copy()
    e[300, env] = 0.0
    assert np.nanmax(e) == 0.0                                         # every other env step is clean, the later ones included
