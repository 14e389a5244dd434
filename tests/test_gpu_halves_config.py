"""GPU: the halves form of the bare one-sub-step launch (csrc/bsk_kernels.hip: SPLIT == 6) OFF the default configuration.

The form carries its own copies of code that reads non-default constants - the phase rule and tick test (``halves_phase_after``,
``halves_fsw_due``: functions of ``fsw_every``), the translational wave's ``rk4_step<PART_TRA>`` and the attitude integrated behind
the hand-over (``h, h2, h3, h6, nmu, j2k``), a second ``BSK_STEP_OUTCOME`` (``reward_mult``, ``failure_penalty``, ``r_min2``,
``inv_wheel_limit``, ``charge_scale``), its own counter word and the raw action integer read by both waves - and every other module
that reaches it (test_gpu_halves*.py, test_gpu_lane_independence.py, test_gpu_bench_shapes.py) runs it at the default constants.
Here every test builds two handles from ONE config, the form forced on and forced off, and after every launch

* compares the two bit for bit (test_gpu_halves._same: state, observations, reward, done, reason, done-mask words, counters,
  batch scalars), and
* compares the halves handle with ``oracle.step`` at the config-space module's tolerances (test_gpu_config_space._check: 1e-11 per
  state field group and observation, 1e-12 reward, reasons and counters exact but for BSK_DONE_ORBIT within a relative 2e-15 of
  r_min, at most 0.1 % of a batch, counted and printed), NOT the tighter ones test_gpu_halves.py measured at the default config,

and asserts the kernel's name through ``CS.kernel_name``.  tests/test_halves_config_host.py shows on the CPU that every one-field
change used here moves the oracle by 1 000 x those tolerances over the same launches, and that the drawn cases end episodes by
LENGTH, ORBIT and WHEELS.  Shapes: 65 (one lane past a workgroup), the ragged 130 / 135 / 200 / 333 / 449, both hub kinds, and one
launch of 256 spacecraft per CU (the upper end of the form's default window).

Measured on an MI355X (``test_zz_worst_errors`` prints them on every run): worst against the oracle over 583 612 spacecraft-steps
- state field group 1.44e-14, observation 5.33e-15, reward 1.11e-16; BSK_DONE_ORBIT ties excused: 0; 3 220 launches compared bit
for bit with the single-wave form, 3 130 of them in the halves kernel, no mismatch: the form is clean off the default config.
Wall time: 2.3 s for the module's 64 tests once the session is up; the largest single tests are a drawn case at 0.27 s, the
541-launch episode at 0.26 s and the 65 536-spacecraft launches at 0.12 s.
"""
import time

import numpy as np
import pytest

import _config_space as CS
import test_gpu_config_space as GC
import test_gpu_halves as H
import test_halves_config_host as HC
from basilisk_env_amd._lib import DONE_LENGTH, GRAV_PM_J2, T_SBR
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from oracle import oracle

pytestmark = pytest.mark.gpu

WORST = {"state": 0.0, "obs": 0.0, "reward": 0.0, "orbit_ties": 0, "envs": 0, "launches": 0, "halves_launches": 0}
T0 = [None]


class _Ref(object):
    """The CPU oracle stepped launch by launch from given counters, with the masked reset of the propagators."""

    def __init__(self, cfg, ic, steps=None, ticks=None, omp=False):
        n = ic.shape[1]
        self.cfg, self.omp, self.st = cfg, omp, np.array(ic, dtype=np.float64, order="C")
        self.steps = np.zeros(n, np.int32) if steps is None else np.array(steps, np.int32)
        self.ticks = np.zeros(n, np.int32) if ticks is None else np.array(ticks, np.int32)

    def step(self, act, k=1):
        """-> the ``ref`` tuple of test_gpu_config_space._check: state, obs, reward, reason, steps, ticks"""
        obs, rew, _, why = oracle.step(self.cfg, self.st, self.steps, self.ticks, act, k, omp=self.omp)
        return self.st, obs, rew, why, self.steps, self.ticks

    def reset(self, fresh, mask):
        m = mask.astype(bool)
        self.st[:, m] = fresh[:, m]
        self.steps[m] = 0
        self.ticks[m] = 0


def _pair(cfg, n, ic, steps=None, ticks=None, force=True):
    """(single-wave handle, halves handle) of one config on one batch, as test_gpu_halves._pair; ``force`` None: the default window."""
    if T0[0] is None:
        T0[0] = time.time()
    a, b = H.make(cfg, n, False), (H.make(cfg, n, True) if force else BatchedPropagator(cfg, n))
    for p in (a, b):
        p.reset(ic)
        p.set_step_stats(True)
        if ticks is not None:
            p.set_counters(np.zeros(n, np.int32) if steps is None else steps, ticks)
    return a, b


def _against_oracle(tag, cfg, b, ref, counters=True):
    st = b.get_state()
    obs, rew, done, why = b.get_obs()
    assert np.array_equal(done, why != 0), tag
    ties = GC.WORST["orbit_ties"]
    GC._check(tag, cfg, st, (obs, rew, why) + (b.get_counters() if counters else ()), ref)
    WORST["state"] = max(WORST["state"], max(GC.max_group_err(st, ref[0], cfg.n_rw).values()))
    WORST["obs"] = max(WORST["obs"], float(np.abs(obs - ref[1]).max()))
    WORST["reward"] = max(WORST["reward"], float(np.abs(rew - ref[2]).max()))
    WORST["orbit_ties"] += GC.WORST["orbit_ties"] - ties
    WORST["envs"] += obs.shape[1]
    return obs, rew, why


def _launch(tag, cfg, a, b, ref, act, k=1, hub="diag", check=True, counters=True):
    """One launch on both handles and the oracle; the two forms bit for bit, the halves handle against the oracle, the names."""
    a.step(act, k)
    b.step(act, k)
    r = ref.step(act, k) if ref is not None else None
    H._same(b, a, tag)
    out = _against_oracle(tag, cfg, b, r, counters) if (check and r is not None) else None
    name = b.kernel_info()["name"]
    assert name == CS.kernel_name(cfg, hub, "bare", "halves" if k == 1 else "single"), (tag, name)
    assert (H._is_halves(b) if k == 1 else H._is_single(b)) and H._is_single(a), (tag, name, a.kernel_info()["name"])
    WORST["launches"] += 1
    WORST["halves_launches"] += int(k == 1)
    return out


def _odd(act):
    return (act < 0) | (act > 2)


# --------------------------------------------------------------------------------------------- A: all constants at once
def test_the_drawn_cells_are_the_halves_modules():
    assert HC.CELLS == H.CELLS


@pytest.mark.parametrize("case", HC.DRAWN, ids=["%d-%s-rw%d-%s" % (s, CS.GRAV_NAME[g], r, h) for s, g, r, h in HC.DRAWN])
def test_all_constants_drawn_in_the_halves_form(case):
    """Every physical constant, ``fsw_every`` (1: every launch hands r, v over; 2, 3, 7, 13), ``dt``, ``fsw_lag`` and ``max_length``
    drawn at once, per-spacecraft tick counters in [0, 100 000) - one wave holds many FSW phases from the first launch - and 48
    launches with a quarter of the actions outside {0, 1, 2}: those earn no reward."""
    seed, grav, n_rw, hub = case
    cfg, ic, ticks0, schedule = HC.drawn_case(*case)
    n = ic.shape[1]
    a, b = _pair(cfg, n, ic, ticks=ticks0)
    ref = _Ref(cfg, ic, ticks=ticks0)
    odd_seen = 0
    for t, (act, k) in enumerate(schedule):
        obs, rew, why = _launch(("all", case, n, t), cfg, a, b, ref, act, k, hub)
        assert (rew[_odd(act)] <= 0.0).all(), (case, t)
        odd_seen += int(_odd(act).sum())
    assert odd_seen > n
    a.close()
    b.close()
    GC._cover([f for f in CS.physical_fields() if any(sc.level == "bare" for sc in CS.FIELDS[f]["live"])],
              "all:" + CS.kernel_name(cfg, hub, "bare", "halves"))


# --------------------------------------------------------------------------------------------- B: one field at a time
@pytest.mark.parametrize("form", ["halves", "halves/fullhub"])
@pytest.mark.parametrize("case", range(len(HC.ONE)), ids=["%s-%s" % (name, sc.name) for name, sc, _ in HC.ONE])
def test_one_field_changed_on_the_halves_form(case, form):
    """One field changed in its bare live scenario (the ``js`` edit follows the hub kind): names the guilty field."""
    name, sc, _, cfg, n, seed, schedule = HC.one_field_pair(case, form)
    hub = "full" if form == "halves/fullhub" else "diag"
    ic = sc.ic(n, seed)
    a, b = _pair(cfg, n, ic)
    ref = _Ref(cfg, ic)
    for t, (act, k) in enumerate(schedule):
        _launch((name, sc.name, form, t), cfg, a, b, ref, act, k, hub)
    a.close()
    b.close()
    GC._cover([name], "one:%s/%s" % (sc.name, form))


# --------------------------------------------------------------------------------------------- C: periods, lags, launch lengths
KS = [1, 1, 1, 4, 1, 1, 7, 1, 1, 1, 2, 1] * 3


@pytest.mark.parametrize("fsw_lag", [0, 1])
@pytest.mark.parametrize("fsw_every", [1, 2, 3, 10, 13])
def test_fsw_periods_and_launch_lengths_interleaved(fsw_every, fsw_lag):
    """One handle alternates between the halves kernel (K = 1) and the single-wave kernel (K = 4, 7, 2): the phase bits of the
    counter word pass between the two forms in both directions.  After the 10th launch a masked reset of lanes 0, 31, 63 and
    n - 1: the restarted lanes run their t = 0 chain on a launch where their neighbours do not."""
    n, n_rw = 65, 4
    cfg = default_config(n_rw, GRAV_PM_J2)
    cfg.fsw_every, cfg.fsw_lag = fsw_every, fsw_lag
    ic = sample_ic_batch(n, n_rw, seed=70 + fsw_every)
    a, b = _pair(cfg, n, ic)
    ref = _Ref(cfg, ic)
    rng = np.random.default_rng(10 * fsw_every + fsw_lag)
    for t, k in enumerate(KS):
        if t == 10:
            mask = np.zeros(n, np.uint8)
            mask[[0, 31, 63, n - 1]] = 1
            fresh = sample_ic_batch(n, n_rw, seed=71 + fsw_every)
            for p in (a, b, ref):
                p.reset(fresh, mask)
        _launch(("interleaved", fsw_every, fsw_lag, t, k), cfg, a, b, ref, rng.integers(0, 3, n).astype(np.int32), k)
    assert np.array_equal(b.get_counters()[1][[0, 1]], [sum(KS[10:]), sum(KS)])
    a.close()
    b.close()


# --------------------------------------------------------------------------------------------- D: the counter word
@pytest.mark.parametrize("fsw_every", [10, 3])
def test_counter_word_edges(fsw_every):
    """Steps at 0xFFFFD .. 0xFFFFF across the lanes and ticks at 10^8 + lane: the step count saturates below the phase bits, the
    tick count advances by one per launch, and each lane's FSW tick falls where ``ticks % fsw_every`` says (the state's
    att_guidance row moves on exactly those launches).  Against the oracle state, observations, rewards and reasons (its step
    count does not saturate); the counters bit for bit against the single-wave form."""
    n, n_rw = 65, 4
    cfg = default_config(n_rw, GRAV_PM_J2)
    cfg.fsw_every = fsw_every
    ic = sample_ic_batch(n, n_rw, seed=80)
    steps0 = (0xFFFFD + np.arange(n) % 3).astype(np.int32)
    ticks0 = (10 ** 8 + np.arange(n)).astype(np.int32)
    a, b = _pair(cfg, n, ic, steps=steps0, ticks=ticks0)
    ref = _Ref(cfg, ic, steps=steps0, ticks=ticks0)
    rng = np.random.default_rng(80)
    sbr = b.get_state()[12 + n_rw + T_SBR].copy()
    ticked = np.zeros(n, bool)
    for t in range(6):
        _, _, why = _launch(("counter word", t), cfg, a, b, ref, rng.integers(0, 3, n).astype(np.int32), counters=False)
        steps, ticks = b.get_counters()
        assert np.array_equal(steps, np.minimum(steps0.astype(np.int64) + t + 1, 0xFFFFF)), t
        assert np.array_equal(ticks, ticks0 + t + 1), t
        assert (why == DONE_LENGTH).all(), t
        now = b.get_state()[12 + n_rw + T_SBR].copy()
        due = (ticks0.astype(np.int64) + t + 1) % fsw_every == 0           # the tick at the END of this launch's sub-step (nav_lag)
        assert np.array_equal(now != sbr, due), (t, np.flatnonzero((now != sbr) != due)[:8])
        ticked |= due
        sbr = now
    assert ticked.any() and not ticked.all() if fsw_every > 6 else ticked.all()
    a.close()
    b.close()


# --------------------------------------------------------------------------------------------- E: the default window
def test_default_window_picks_the_form_under_a_drawn_config():
    """No ``set_halves_form(True)``: at 256 spacecraft per CU (65 536 on a whole MI355X, the benchmark's headline batch) the library
    itself picks the form, under a drawn config; three launches with mixed actions, the oracle on every spacecraft."""
    n, n_rw = 256 * H._device_cus(), 4
    rng = np.random.default_rng(4096)
    cfg = CS.draw_config(rng, n_rw, GRAV_PM_J2, "bare", "diag")
    CS.draw_halves_structure(cfg, rng)
    cfg.fsw_every = 3                                      # launch 1 carries the regular hand-over, launch 0 the t = 0 chain
    ic = sample_ic_batch(n, n_rw, seed=4096)
    a, b = _pair(cfg, n, ic, force=None)
    ref = _Ref(cfg, ic, omp=True)
    for t in range(3):
        act = ((np.arange(n) * 7 + t) % 3).astype(np.int32)
        act[t::97] = 255
        _, rew, _ = _launch(("window", n, t), cfg, a, b, ref, act)
        assert (rew[_odd(act)] <= 0.0).all(), t
        assert b.kernel_info()["name"].endswith(",halves>")
    a.close()
    b.close()


# --------------------------------------------------------------------------------------------- F: a whole episode
def test_whole_episode_in_one_sub_step_launches():
    """541 launches of one sub-step under a drawn config, ``max_length = 540``: halves against single-wave bit for bit after every
    launch; the oracle on launches 0 - 99 (the config-space tolerances are known to hold within 100 sub-steps of a reset: that
    module's schedules run 102; beyond, the single-wave form is the reference, which tests/test_gpu_episode.py ties to the oracle
    over whole episodes).  Every spacecraft ends by LENGTH at the last launch and none earlier."""
    n, n_rw = 130, 4
    rng = np.random.default_rng(540)
    cfg = CS.draw_config(rng, n_rw, GRAV_PM_J2, "bare", "diag")
    CS.draw_halves_structure(cfg, rng)
    cfg.max_length = 540
    ic = sample_ic_batch(n, n_rw, seed=540)
    a, b = _pair(cfg, n, ic)
    ref = _Ref(cfg, ic)
    for t in range(541):
        act = rng.integers(0, 3, n).astype(np.int32)
        _launch(("episode", t), cfg, a, b, ref if t < 100 else None, act)
        length = (b.get_obs()[3] & DONE_LENGTH) != 0
        assert length.all() if t == 540 else not length.any(), t
    assert np.array_equal(b.get_counters()[0], np.full(n, 541))
    a.close()
    b.close()


# --------------------------------------------------------------------------------------------- what was seen
def test_zz_worst_errors(capsys):
    """Prints the worst error per quantity against the oracle, the BSK_DONE_ORBIT ties excused (counted; capped at 0.1 %), the
    module's wall time and the fields varied on the halves form (the module docstring records one run's figures)."""
    with capsys.disabled():
        print("\nhalves form off the default config, worst against the oracle: state group %.2e (< 1e-11), observation %.2e (< 1e-11), reward %.2e (< 1e-12)"
              % (WORST["state"], WORST["obs"], WORST["reward"]))
        print("BSK_DONE_ORBIT ties excused: %d of %d spacecraft-steps (%.4f %%); %d launches compared bit for bit with the single-wave form, %d of them in the halves kernel"
              % (WORST["orbit_ties"], WORST["envs"], 100.0 * WORST["orbit_ties"] / max(WORST["envs"], 1), WORST["launches"], WORST["halves_launches"]))
        if T0[0] is not None:
            print("wall time since the module's first handle: %.1f s" % (time.time() - T0[0]))
        for name in CS.physical_fields():
            labels = sorted(l for l in GC.COVER.get(name, ()) if "halves" in l)
            if labels:
                print("%-18s %3d  %s" % (name, len(labels), "; ".join(labels[:4]) + (" ..." if len(labels) > 4 else "")))
    assert WORST["orbit_ties"] <= 1e-3 * max(WORST["envs"], 1)
