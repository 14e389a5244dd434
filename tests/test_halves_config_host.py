"""CPU: the power of tests/test_gpu_halves_config.py, which holds the halves form of the one-sub-step launch to the oracle off
the default configuration.  Nothing here runs a kernel.  On the schedule of one-sub-step launches that form runs
(``CS.halves_schedule``): every bare one-field change with wheels moves the oracle's outputs by 1 000 x the GPU tolerances
(``CS.LIVE``); the drawn cases stay finite, keep clear of the BSK_DONE_ORBIT tie rule and end episodes by LENGTH, ORBIT and
WHEELS; and an action outside {0, 1, 2} earns no reward.  ``drawn_case`` is what the GPU module runs, draw for draw."""
import numpy as np
import pytest

import _config_space as CS
from basilisk_env_amd._lib import DONE_LENGTH, DONE_ORBIT, DONE_WHEELS, GRAV_PM, GRAV_PM_J2
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from helpers import general_hub

# tests/test_gpu_halves.py: CELLS (the GPU module asserts that the two lists are one)
CELLS = [(GRAV_PM_J2, 4, "diag"), (GRAV_PM, 3, "diag"), (GRAV_PM_J2, 3, "full"), (GRAV_PM, 4, "full")]
SEEDS = 3
DRAWN = [(seed,) + cell for cell in CELLS for seed in range(SEEDS)]
TIE = 2e-15                            # |r| / r_min - 1 inside which r.r < r_min^2 and |r| < r_min may round apart
ONE = [(name, sc, edit) for name, sc, _, edit in CS.one_field_cases() if sc.level == "bare" and sc.n_rw > 0]


def drawn_case(seed, grav, n_rw, hub):
    """Every physical constant and the halves form's structure fields drawn at once -> cfg, ic, ticks0 (per spacecraft, so that one
    wave holds many FSW phases from the first launch), 48 launches with a quarter of the actions out of range."""
    rng = np.random.default_rng([seed, n_rw, grav, int(hub == "diag"), 6])
    cfg = CS.draw_config(rng, n_rw, grav, "bare", hub)
    CS.draw_halves_structure(cfg, rng)
    n = int(rng.choice([65, 130, 200, 333, 449]))                       # ragged tails
    ic = sample_ic_batch(n, n_rw, seed=int(rng.integers(1 << 30)))
    ic[12:12 + n_rw] *= rng.uniform(0.5, 2.5)
    ticks0 = rng.integers(0, 100000, n).astype(np.int32)
    return cfg, ic, ticks0, CS.halves_schedule(n, int(rng.integers(1 << 30)), odd_actions=True)


def one_field_pair(case, form):
    """-> name, scenario, (config, edited config) of a bare one-field case on ``halves`` or ``halves/fullhub``; n, seed, schedule."""
    name, sc, edit = ONE[case]
    base = sc.config()
    if form == "halves/fullhub":
        general_hub(base)
    edited = edit(CS.copy_into(sc.config(), base), "fullhub" if form == "halves/fullhub" else "single")
    n, seed = 135, 1 + case % 3
    return name, sc, base, edited, n, seed, CS.halves_schedule(n, seed)


@pytest.mark.parametrize("form", ["halves", "halves/fullhub"])
@pytest.mark.parametrize("case", range(len(ONE)), ids=["%s-%s" % (name, sc.name) for name, sc, _ in ONE])
def test_every_bare_one_field_change_is_visible_over_one_sub_step_launches(case, form, capsys):
    name, sc, base, edited, n, seed, schedule = one_field_pair(case, form)
    ic = sc.ic(n, seed)
    c = CS.change(CS.run_oracle(base, ic, schedule), CS.run_oracle(edited, ic, schedule), sc.n_rw)
    with capsys.disabled():
        print("\n%-18s %-22s %-15s state %.2e obs %.2e reward %.2e reason %.3f" % (name, sc.name, form, c["state"], c["obs"], c["reward"], c["reason"]), end="")
    if CS.FIELDS[name]["invariant"]:                # ctrl_axes: dead by algebra (tests/test_config_space_host.py asserts it invariant)
        assert name == "ctrl_axes"
        return
    assert CS.is_live(c), (name, sc.name, form, c)


def test_there_are_seventeen_live_bare_one_field_cases_with_wheels():
    assert len([1 for name, _, _ in ONE if not CS.FIELDS[name]["invariant"]]) == 17 and len(ONE) == 18


_RUNS = {}


def _drawn_run(case):
    if case not in _RUNS:
        cfg, ic, ticks0, schedule = drawn_case(*case)
        _RUNS[case] = (cfg, schedule, CS.run_oracle(cfg, ic, schedule, ticks0=ticks0))
    return _RUNS[case]


@pytest.mark.parametrize("case", DRAWN, ids=["%d-%s-rw%d-%s" % (s, CS.GRAV_NAME[g], r, h) for s, g, r, h in DRAWN])
def test_drawn_cases_stay_finite_and_clear_of_orbit_ties(case):
    cfg, schedule, out = _drawn_run(case)
    ties = total = 0
    seen = 0
    for (act, _), (st, obs, rew, why, _, _) in zip(schedule, out):
        assert np.isfinite(st).all() and np.isfinite(obs).all() and np.isfinite(rew).all()
        ties += int((np.abs(np.linalg.norm(st[0:3], axis=0) / cfg.r_min - 1.0) < TIE).sum())
        total += act.size
        seen |= int(np.bitwise_or.reduce(why))
        assert (rew[(act < 0) | (act > 2)] <= 0.0).all()
    assert ties < 1e-3 * total, (ties, total)
    assert seen & DONE_LENGTH and seen & DONE_ORBIT, seen
    assert out[0][5].min() != out[0][5].max() and len(set(out[0][5] % cfg.fsw_every)) == min(cfg.fsw_every, 13)


def test_drawn_cases_together_end_episodes_by_length_orbit_and_wheels():
    seen, periods, lags = 0, set(), set()
    for case in DRAWN:
        cfg, _, out = _drawn_run(case)
        seen |= int(np.bitwise_or.reduce([np.bitwise_or.reduce(o[3]) for o in out]))
        periods.add(cfg.fsw_every)
        lags.add(cfg.fsw_lag)
    assert seen & DONE_LENGTH and seen & DONE_ORBIT and seen & DONE_WHEELS, seen
    assert 1 in periods and len(periods) >= 3 and lags == {0, 1}, (periods, lags)      # every launch an FSW launch is among the draws


def test_out_of_range_actions_earn_no_reward():
    """``oracle/bsk_oracle.c: guidance`` treats every action other than 0 as the inertial target, and only action 0 is rewarded: under
    the default and a drawn config (failure_penalty != 1, another reward_mult), every raw integer of ``CS.ODD_ACTIONS``."""
    from basilisk_env_amd.simulators.dynamics.config import default_config
    n = 6 * len(CS.ODD_ACTIONS)
    act = np.repeat(np.array(CS.ODD_ACTIONS, np.int32), 6)
    for cfg in (default_config(4, GRAV_PM_J2), drawn_case(0, *CELLS[0])[0]):
        ic = sample_ic_batch(n, 4, seed=3)
        odd = CS.run_oracle(cfg, ic, [(act, 1)] * 12)
        one = CS.run_oracle(cfg, ic, [(np.ones(n, np.int32), 1)] * 12)
        for (st, obs, rew, why, _, _), (st1, obs1, rew1, why1, _, _) in zip(odd, one):
            assert (rew <= 0.0).all()
            assert np.array_equal(st, st1) and np.array_equal(obs, obs1) and np.array_equal(rew, rew1) and np.array_equal(why, why1)
