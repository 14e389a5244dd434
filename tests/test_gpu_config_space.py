"""GPU: every physical constant of ``bsk_config`` away from its default, in every kernel form, against the CPU oracle.

``build_params`` (csrc/bsk_config.hip) hands the kernels several derived copies of most constants (``js`` alone lives in
``StepParams.js``, ``ColdCfg.js`` and four rows of the broadcast table), different kernel forms read different copies, and
``bsk_default_config`` is symmetric exactly where an indexing mistake would show.  tests/_config_space.py classifies every field
and says how to draw it asymmetrically; tests/test_config_space_host.py shows that the oracle agrees with the 50-digit model over
those draws and that every one-field change below moves the oracle's outputs by 1 000 x the tolerances used here.  This module:

* ``test_all_constants_drawn_*``: every constant drawn at once, on every form tests/test_gpu_kernel_info.py::STEPPED pins, the
  fused rollout kernel (every history row), the ``bsk_step_n`` fallback and block 256 above 2^20 spacecraft;
* ``test_one_field_*``: one field changed in its live scenario, on every form that reads a copy of it - names the guilty field;
* ``test_done_reasons_*``: BSK_DONE_ORBIT for half of a batch, two, three and four reasons on one step with failure_penalty != 1,
  the done-mask words and the batch scalars;
* ``test_reset_*`` / ``test_device_sampler_*`` / ``test_forked_*``: the other consumers of the config.

All through the C-ABI, reference = ``oracle.step``; tolerances are the project's own (tests/test_gpu_fuzz.py): 1e-11 per state field
group and observation, 1e-12 reward, 1e-7 W s battery, reasons and counters bit for bit.  The kernels compare r.r with r_min^2, the
oracle |r| with r_min: a spacecraft within a relative 2e-15 of r_min may go either way (at most 0.1 % of a batch; printed).
The last test prints the coverage table (field -> forms it was varied on) and the worst error seen per quantity.

Wall time on an MI355X: 8 s for the module's 136 tests once the session is up (the library build and the first use of the device,
which every session pays, took another 37 s when this module ran alone); the largest single test is block 256 at 0.6 s.  Nothing
was cut: three seeds per pinned form, every one-field case on every form listed for its level.
"""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import _config_space as CS
import test_gpu_kernel_info as KI
from _oracle_backend import OraclePropagator
from basilisk_env_amd import _hip
from basilisk_env_amd._lib import (DONE_BATTERY, DONE_LENGTH, DONE_ORBIT, DONE_WHEELS, FLAG_AUTO_RESET, FLAG_LDS_SCRATCH, FLAG_POWER,
                                   GRAV_PM, GRAV_PM_J2, GRAV_SH, T_CHARGE)
from basilisk_env_amd.simulators.dynamics import BatchedPropagator
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from helpers import general_hub, max_group_err, visible_sh_coefficients

pytestmark = pytest.mark.gpu

SEEDS = 3                              # per kernel form, all constants drawn at once
WORST = {"state": 0.0, "charge": 0.0, "obs": 0.0, "reward": 0.0, "orbit_ties": 0, "envs": 0}
COVER = {}                             # field -> set of form labels it was varied on (away from its default)
RAN = set()


@contextlib.contextmanager
def _switches(pair="0", tri="0", sh_form=None):
    env = {"BSKGPU_PAIR": pair, "BSKGPU_TRI": tri, "BSKGPU_SH_FORM": sh_form}
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _propagator(cfg, n, pair="0", tri="0", sh_form=None, sh=(None, None)):
    with _switches(pair, tri, sh_form):
        prop = BatchedPropagator(cfg, n)
        if cfg.gravity_model == GRAV_SH:
            prop.set_gravity_sh(cfg.sh_degree, sh[0], sh[1])
    return prop


def _cover(fields, label):
    for f in fields:
        COVER.setdefault(f, set()).add(label)


def _check(tag, cfg, got_state, got, ref):
    """One env step's outputs against the oracle's: (obs, reward, reason[, steps, ticks]) and, if given, the state."""
    st, obs, rew, why, steps, ticks = ref
    n_rw, n = cfg.n_rw, obs.shape[1]
    if got_state is not None:
        errs = max_group_err(got_state, st, n_rw)
        WORST["state"] = max(WORST["state"], max(errs.values()))
        assert max(errs.values()) < 1e-11, (tag, errs)
        if cfg.flags & FLAG_POWER:
            dq = float(np.abs(got_state[12 + n_rw + T_CHARGE] - st[12 + n_rw + T_CHARGE]).max())
            WORST["charge"] = max(WORST["charge"], dq)
            assert dq < 1e-7, (tag, dq)
    eo, er = float(np.abs(got[0] - obs).max()), float(np.abs(got[1] - rew).max())
    WORST["obs"], WORST["reward"] = max(WORST["obs"], eo), max(WORST["reward"], er)
    assert eo < 1e-11, (tag, eo, np.abs(got[0] - obs).max(axis=1))
    assert er < 1e-12, (tag, er)
    diff = np.flatnonzero(got[2] != why)
    if diff.size:       # only BSK_DONE_ORBIT, only within the rounding of r.r < r_min^2 against |r| < r_min
        r = np.linalg.norm(st[0:3, diff], axis=0)
        assert np.all((got[2][diff] ^ why[diff]) == DONE_ORBIT) and np.all(np.abs(r / cfg.r_min - 1.0) < 2e-15), (tag, diff[:8], got[2][diff][:8], why[diff][:8])
        assert diff.size <= 1e-3 * n, (tag, diff.size, n)
        WORST["orbit_ties"] += int(diff.size)
    WORST["envs"] += n
    if len(got) > 3:
        assert np.array_equal(got[3], steps) and np.array_equal(got[4], ticks), tag


def _run_steps(tag, cfg, prop, ic, schedule, sim_time0=0.0, sh=(None, None), ticks0=0, want=None, omp=False):
    n = ic.shape[1]
    prop.reset(ic)
    if ticks0:
        prop.set_counters(np.zeros(n, np.int32), np.full(n, ticks0, np.int32))
    if sim_time0:
        prop.set_sim_time(sim_time0)
    ref = CS.run_oracle(cfg, ic, schedule, sim_time0, sh, ticks0, omp=omp)
    for call, ((act, k), r) in enumerate(zip(schedule, ref)):
        prop.step(act, k)
        obs, rew, done, why = prop.get_obs()
        assert np.array_equal(done, why != 0), tag
        _check(tag + (call, k), cfg, prop.get_state(), (obs, rew, why) + prop.get_counters(), r)
        if want:
            assert prop.kernel_info()["name"] == want, (tag, prop.kernel_info()["name"], want)
    return ref


def _run_rollout(tag, cfg, prop, ic, schedule, constant, want):
    """The schedule's actions (or one constant action) at its first call's sub-step count, in ONE launch: every history row."""
    T, k, n = len(schedule), schedule[0][1], ic.shape[1]
    acts = np.stack([np.full(n, constant, np.int32) if constant is not None else a for a, _ in schedule])
    prop.reset(ic)
    ref = CS.run_oracle(cfg, ic, [(acts[t], k) for t in range(T)])
    obs, rew, why = prop.rollout(T, k, actions=None if constant is not None else acts, constant_action=constant or 0)
    for t in range(T):
        _check(tag + ("row", t), cfg, None, (obs[t], rew[t], why[t]), ref[t])
    last = prop.get_obs()
    _check(tag + ("final",), cfg, prop.get_state(), (last[0], last[1], last[3]) + prop.get_counters(), ref[-1])
    assert prop.kernel_info()["name"] == want, (tag, prop.kernel_info()["name"], want)


def _drawn_case(seed, n_rw, grav, level, diag, salt):
    rng = np.random.default_rng([seed, n_rw, grav, LEVEL_NO[level], int(diag), salt])
    cfg = CS.draw_config(rng, n_rw, grav, level, "diag" if diag else "full")
    n = int(rng.choice([65, 130, 200, 333, 449]))                       # ragged tails
    ic = sample_ic_batch(n, n_rw, seed=int(rng.integers(1 << 30)))
    if n_rw:
        ic[12:12 + n_rw] *= rng.uniform(0.5, 2.5)
    schedule = [(rng.integers(0, 3, n).astype(np.int32), int(rng.integers(1, 48))) for _ in range(3)]
    sh = visible_sh_coefficients(CS.SH_DEGREE, seed=seed) if grav == GRAV_SH else (None, None)
    return cfg, ic, schedule, sh


LEVEL_NO = {name: i for i, name in enumerate(CS.LEVELS)}


# --------------------------------------------------------------------------------------------- all constants at once
@pytest.mark.parametrize("case", range(len(KI.STEPPED)), ids=[w[0] for _, w in KI.STEPPED])
def test_all_constants_drawn_on_every_pinned_step_kernel_form(case):
    (grav, n_rw, level, diag, pair, tri, sh_form), (want, _, _) = KI.STEPPED[case]
    for seed in range(SEEDS):
        cfg, ic, schedule, sh = _drawn_case(seed, n_rw, grav, level, diag, 0)
        prop = _propagator(cfg, ic.shape[1], pair, tri, sh_form, sh)
        _run_steps((want, seed, ic.shape[1]), cfg, prop, ic, schedule, sh=sh, want=want)
        prop.close()
    # a field counts as varied on this form if one of its live scenarios is at or below the form's level (harmonics-only fields: on harmonics)
    live = [f for f in CS.physical_fields() if any(LEVEL_OF[sc.level] <= LEVEL_OF[level] and (sc.level != "sh" or grav == GRAV_SH) for sc in CS.FIELDS[f]["live"])]
    if n_rw == 0:
        live = [f for f in live if f not in WHEEL_FIELDS]
    _cover(live, "all:" + want)
    RAN.add(("all", case))


WHEEL_FIELDS = ("js", "u_max", "u_min", "f_coulomb", "K", "P", "ctrl_axes", "wheel_limit", "n_thr", "thr_max_counter", "thr_pos", "thr_dir",
                "thr_max_thrust", "thr_min_fire_time", "thr_min_on_time", "hs_min")
LEVEL_OF = {"bare": 0, "ldss": 0, "sh": 0, "power": 1, "full": 2, "fullg": 2}

ROLLOUTS = [(GRAV_PM_J2, 4, True, 1), (GRAV_PM, 3, False, None), (GRAV_PM, 0, True, None), (GRAV_PM_J2, 3, True, 0), (GRAV_PM_J2, 4, False, 2)]


@pytest.mark.parametrize("grav,n_rw,diag,constant", ROLLOUTS)
def test_all_constants_drawn_in_the_fused_rollout_kernel(grav, n_rw, diag, constant):
    want = CS.kernel_name(CS.draw_config(np.random.default_rng(0), n_rw, grav, "bare"), "diag" if diag else "full", "bare",
                          rollout="constant" if constant is not None else "actions")
    for seed in range(SEEDS):
        cfg, ic, schedule, _ = _drawn_case(seed, n_rw, grav, "bare", diag, 1)
        schedule = schedule + [(np.roll(a, 1), k) for a, k in schedule]          # six env steps in the launch
        prop = _propagator(cfg, ic.shape[1])
        _run_rollout((want, seed), cfg, prop, ic, schedule, constant, want)
        prop.close()
    _cover([f for f in CS.physical_fields() if any(sc.level in ("bare",) for sc in CS.FIELDS[f]["live"])], "all:" + want)
    RAN.add(("rollout", grav, n_rw, diag))


FALLBACKS = [((GRAV_PM_J2, 3, "full", True, "0", "1", None), "step_kernel<PM_J2,3,diag,scenario,tri>"),
             ((GRAV_SH, 0, "bare", True, "0", "0", "5"), "step_kernel<SH/dpp2,0,diag>"),
             ((GRAV_PM, 4, "ldss", False, "0", "0", None), "step_kernel<PM,4,full,lds-scratch>")]


@pytest.mark.parametrize("case", range(len(FALLBACKS)), ids=[w for _, w in FALLBACKS])
def test_all_constants_drawn_where_step_n_falls_back_to_single_launches(case):
    (grav, n_rw, level, diag, pair, tri, sh_form), want = FALLBACKS[case]
    cfg, ic, schedule, sh = _drawn_case(0, n_rw, grav, level, diag, 2)
    n, k = ic.shape[1], schedule[0][1]
    prop = _propagator(cfg, n, pair, tri, sh_form, sh)
    prop.reset(ic)
    acts = np.stack([a for a, _ in schedule])
    ref = CS.run_oracle(cfg, ic, [(a, k) for a in acts], sh=sh)
    obs, rew, why = prop.rollout(len(schedule), k, actions=acts)
    for t in range(len(schedule)):
        _check((want, "row", t), cfg, None, (obs[t], rew[t], why[t]), ref[t])
    _check((want, "final"), cfg, prop.get_state(), (obs[-1], rew[-1], why[-1]) + prop.get_counters(), ref[-1])
    assert prop.kernel_info()["name"] == want
    prop.close()


def test_all_constants_drawn_at_block_256_above_2_to_the_20():
    """Batches of 2^20 spacecraft and more launch 256-lane workgroups below the power level (csrc/bsk_capi.hip: bsk_create): one drawn
    config, one call of 7 sub-steps; the oracle on every host core."""
    n, n_rw = (1 << 20) + 37, 4
    cfg = CS.draw_config(np.random.default_rng(256), n_rw, GRAV_PM_J2, "bare", "diag")
    ic = sample_ic_batch(n, n_rw, seed=256)
    prop = _propagator(cfg, n)
    _run_steps(("block256",), cfg, prop, ic, [((np.arange(n) % 3).astype(np.int32), 7)], omp=True)
    info = prop.kernel_info()
    assert (info["name"], info["block"]) == ("step_kernel<PM_J2,4,diag>", 256), info
    prop.close()


# --------------------------------------------------------------------------------------------- one field at a time
ONE = CS.one_field_cases()


def _form_setup(sc, form, cfg):
    """-> (hub, level, pair, tri, sh_form, rollout) of a form label; edits ``cfg`` where the form is a property of the config."""
    hub, level, pair, tri, sh_form, rollout = "diag", sc.level, "0", "0", None, None
    if form == "fullhub":
        general_hub(cfg)
        hub = "full"
    elif form == "ldss":
        cfg.flags |= FLAG_LDS_SCRATCH
        level = "ldss"
    elif form == "generic":
        CS.generic_facets(cfg, np.random.default_rng(5))
        level = "fullg"
    elif form == "pair":
        pair = "1"
    elif form == "tri":
        tri = "1"
    elif form == "rollout":
        rollout = "actions"
    elif form in ("sh1", "sh4", "sh5"):
        sh_form, level = form[2], "bare"
    return hub, level, pair, tri, sh_form, rollout


@pytest.mark.parametrize("case", range(len(ONE)), ids=["%s-%s" % (name, sc.name) for name, sc, _, _ in ONE])
def test_one_field_changed_in_its_live_scenario_on_every_form_that_reads_it(case):
    name, sc, forms, edit = ONE[case]
    n, seed = 135, 1 + case % 3
    ic, schedule, sh = sc.ic(n, seed), sc.schedule(n, seed), sc.sh()
    for form in forms:
        cfg = sc.config()
        hub, level, pair, tri, sh_form, rollout = _form_setup(sc, form, cfg)
        edit(cfg, form)
        tag = (name, sc.name, form)
        prop = _propagator(cfg, n, pair, tri, sh_form, sh)
        if rollout:
            _run_rollout(tag, cfg, prop, ic, schedule, None, CS.kernel_name(cfg, hub, level, rollout=rollout))
        else:
            _run_steps(tag, cfg, prop, ic, schedule, sc.sim_time0, sh, sc.ticks0, want=CS.kernel_name(cfg, hub, level, form if form in ("pair", "tri") else "single", sh_form))
        prop.close()
        _cover([name], "one:%s/%s" % (sc.name, form))
    RAN.add(("one", case))


# --------------------------------------------------------------------------------------------- done reasons, rewards
def _dev_array(view, dtype, count):
    out = np.empty(count, dtype=dtype)
    ptr = view.__cuda_array_interface__["data"][0]
    _hip.check(_hip.runtime().hipMemcpyAsync(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), out.nbytes, _hip.hipMemcpyDeviceToHost, ctypes.c_void_p(0)), "hipMemcpyAsync")
    _hip.stream_sync(0)
    return out


def _failing_case(level, n):
    sc = CS.Scenario(level, ("failures",))
    cfg = sc.config()
    CS._one_r_min(cfg, None, None)
    cfg.failure_penalty = 0.37
    cfg.max_length = 1                                  # the second env step ends every episode by length as well
    return sc, cfg, sc.ic(n, 4)


@pytest.mark.parametrize("level,form", [("bare", "single"), ("bare", "ldss"), ("bare", "fullhub"), ("power", "single"), ("power", "pair"),
                                         ("full", "single"), ("full", "pair"), ("full", "tri"), ("full", "generic")])
def test_done_reasons_rewards_mask_and_batch_scalars_off_the_default(level, form):
    n = 1000
    sc, cfg, ic = _failing_case(level, n)
    hub, lvl, pair, tri, sh_form, _ = _form_setup(sc, form, cfg)
    schedule = sc.schedule(n, 4)[:2]
    prop = _propagator(cfg, n, pair, tri)
    prop.reset(ic)
    ref = CS.run_oracle(cfg, ic, schedule)
    for call, ((act, k), r) in enumerate(zip(schedule, ref)):
        prop.step(act, k)
        obs, rew, done, why = prop.get_obs()
        tag = (level, form, call)
        _check(tag, cfg, prop.get_state(), (obs, rew, why) + prop.get_counters(), r)
        mask = _dev_array(prop.device_views()["done_mask"], np.uint64, (n + 63) // 64)
        bits = ((mask[np.arange(n) // 64] >> (np.arange(n) % 64).astype(np.uint64)) & np.uint64(1)).astype(bool)
        assert np.array_equal(bits, why != 0), tag
        rsum, ndone = prop.batch_stats()
        # each reward is within 1e-12 of the oracle's: so is their sum within n x 1e-12 (the summation order adds ~1e-13 at this size)
        assert ndone == int((why != 0).sum()) and abs(rsum - float(r[2].sum())) < n * 1e-12, (tag, rsum, float(r[2].sum()))
    first, second = ref[0][3], ref[1][3]
    orbit = ((first & DONE_ORBIT) != 0).mean()
    assert 0.3 < orbit < 0.7, orbit                                    # BSK_DONE_ORBIT for roughly half of the batch
    nbits = np.array([bin(int(w)).count("1") for w in second])
    assert (second & DONE_LENGTH).all() and (nbits == 2).any() and (nbits == 3).any()
    if level == "bare":
        assert (second == (DONE_LENGTH | DONE_WHEELS | DONE_BATTERY | DONE_ORBIT)).any() and (nbits == 4).sum() >= 5
    two_fail = (second & (DONE_WHEELS | DONE_BATTERY)) == (DONE_WHEELS | DONE_BATTERY)
    if level == "bare":
        assert two_fail.any() and np.all(ref[1][2][two_fail] < -2 * 0.37 + 1.0 / 540.0 + 1e-12)
    assert prop.kernel_info()["name"] == CS.kernel_name(cfg, hub, lvl, form if form in ("pair", "tri") else "single")
    prop.close()
    _cover(["r_min", "failure_penalty"], "done:%s/%s" % (level, form))


@pytest.mark.parametrize("constant", [None, 0])
def test_done_reasons_and_rewards_off_the_default_in_the_rollout_kernel(constant):
    n = 1000
    sc, cfg, ic = _failing_case("bare", n)
    schedule = [(a, 23) for a, _ in sc.schedule(n, 4)]
    prop = _propagator(cfg, n)
    want = CS.kernel_name(cfg, "diag", "bare", rollout="constant" if constant is not None else "actions")
    _run_rollout(("done-rollout", constant), cfg, prop, ic, schedule, constant, want)
    acts = [np.full(n, constant, np.int32) if constant is not None else a for a, _ in schedule]
    ref = CS.run_oracle(cfg, ic, [(a, 23) for a in acts])
    assert (ref[1][3] == 15).any() and 0.3 < ((ref[0][3] & DONE_ORBIT) != 0).mean() < 0.7
    prop.close()
    _cover(["r_min", "failure_penalty"], "done:" + want)


# --------------------------------------------------------------------------------------------- the other consumers
def _initial_obs(cfg, ic):
    """What a reset leaves as the first observation (envs/leoPowerAttitudeVecEnv.py: _initial_obs), from the drawn config."""
    n_rw, t = cfg.n_rw, 12 + cfg.n_rw
    ob = np.empty((5, ic.shape[1]))
    ob[0], ob[1] = np.linalg.norm(ic[6:9], axis=0), np.linalg.norm(ic[9:12], axis=0)
    ob[2] = np.linalg.norm(ic[12:12 + n_rw], axis=0) / cfg.wheel_limit if n_rw else 0.0
    ob[3] = ic[t + T_CHARGE] / 3600.0 / cfg.power_max
    ob[4] = 1.0
    return ob


@pytest.mark.parametrize("n_rw,level", [(4, "bare"), (3, "power"), (0, "bare"), (4, "full")])
def test_reset_and_device_auto_reset_outputs_under_a_drawn_config(n_rw, level):
    """init_outputs_kernel and the step kernel's restart epilogue read wheel_limit and power_max (ResetOut): host reset, masked
    reset and restarts from the pool inside the launch, against the mirror / the oracle-backed propagator."""
    n = 270
    cfg = CS.draw_config(np.random.default_rng(77 + n_rw), n_rw, GRAV_PM_J2, level, "diag")
    cfg.flags |= FLAG_AUTO_RESET
    cfg.max_length = 1
    ic, pool = sample_ic_batch(n, n_rw, seed=5), sample_ic_batch(41, n_rw, seed=6)
    g, c = BatchedPropagator(cfg, n), OraclePropagator(cfg, n)
    for p in (g, c):
        p.set_ic_pool(pool)
        p.reset(ic)
    obs, rew, done, why = g.get_obs()
    assert np.allclose(obs, _initial_obs(cfg, ic), rtol=1e-15, atol=0) and not rew.any() and not why.any()
    rng = np.random.default_rng(n_rw)
    restarts = 0
    for step in range(4):
        act = rng.integers(0, 2, n).astype(np.int32)
        g.step(act, 6)
        c.step(act, 6)
        og, rg, dg, wg = g.get_obs()
        oc, rc, dc, wc = c.get_obs()
        assert np.array_equal(wg, wc), step
        assert np.abs(og - oc).max() < 1e-11 and np.abs(rg - rc).max() < 1e-12, (step, np.abs(og - oc).max(axis=1))
        assert max(max_group_err(g.get_state(), c.get_state(), n_rw).values()) < 1e-11
        assert np.array_equal(g.get_state()[:, dg], c.get_state()[:, dc])          # restarted envs hold the pool's values exactly
        tg, eg = g.get_terminal_obs()
        tc, ec = c.get_terminal_obs()
        assert np.array_equal(eg, ec) and (not dg.any() or np.abs(tg[:, dg] - tc[:, dc]).max() < 1e-11)
        restarts += int(dg.sum())
    assert restarts >= n
    mask = (np.arange(n) % 3 == 1).astype(np.uint8)
    ic2 = sample_ic_batch(n, n_rw, seed=8)
    g.reset(ic2, mask)
    m = mask.astype(bool)
    assert np.allclose(g.get_obs()[0][:, m], _initial_obs(cfg, ic2)[:, m], rtol=1e-15, atol=0)
    g.close()
    _cover(["wheel_limit", "power_max"], "reset/auto-reset outputs (%s, %d wheels)" % (level, n_rw))


@pytest.mark.parametrize("n_rw,factor", [(0, 0.9), (4, 1.1)])
def test_device_sampler_with_a_non_default_mu(n_rw, factor):
    """sample_pool_kernel takes mu from the config: orbits of the SAME elements have other speeds (tests/_philox_ref.py)."""
    from _philox_ref import sample_pool
    from basilisk_env_amd.simulators.dynamics import default_config
    cfg = default_config(n_rw, GRAV_PM)
    cfg.flags |= FLAG_AUTO_RESET
    cfg.mu *= factor
    p = BatchedPropagator(cfg, 64)
    p.sample_ic_pool(300, seed=0xABCDEF0123456789)
    got = p.get_ic_pool()
    ref = sample_pool(300, n_rw, 0xABCDEF0123456789, mu=cfg.mu)
    dflt = sample_pool(300, n_rw, 0xABCDEF0123456789)
    for sl in (slice(0, 3), slice(3, 6), slice(6, 9), slice(9, 12), slice(12, None)):
        scale = np.maximum(np.abs(ref[sl]).max(axis=0), 1e-300)
        assert (np.abs(got[sl] - ref[sl]).max(axis=0) / scale).max() < 1e-14, sl
    assert np.abs(ref[3:6] - dflt[3:6]).max() / np.abs(dflt[3:6]).max() > 0.03            # (the test has power: v follows sqrt(mu))
    p.close()
    _cover(["mu"], "device IC sampler (%d wheels)" % n_rw)


@pytest.mark.parametrize("level,pair,tri", [("bare", "0", "0"), ("full", "0", "1")])
def test_forked_children_carry_the_drawn_config(level, pair, tri):
    """bsk_fork_device copies states between handles of one config: a child created with a drawn config and filled from a parent
    steps like the oracle under THAT config (parent stepped first, three children per parent, other actions)."""
    n_rw, n = 4, 97
    cfg = CS.draw_config(np.random.default_rng(31), n_rw, GRAV_PM_J2, level, "diag")
    ic = sample_ic_batch(n, n_rw, seed=12)
    parent = _propagator(cfg, n, pair, tri)
    child = _propagator(cfg, 3 * n, pair, tri)
    rng = np.random.default_rng(3)
    act0 = rng.integers(0, 3, n).astype(np.int32)
    parent.reset(ic)
    child.reset(sample_ic_batch(3 * n, n_rw, seed=13))
    ref = CS.run_oracle(cfg, ic, [(act0, 17)])[0]
    parent.step(act0, 17)
    idx = np.repeat(np.arange(n), 3).astype(np.int32)
    child.fork_from(parent, idx)
    st = np.ascontiguousarray(ref[0][:, idx])
    steps, ticks = ref[4][idx].copy(), ref[5][idx].copy()
    from oracle import oracle
    for call in range(2):
        act, k = rng.integers(0, 3, 3 * n).astype(np.int32), int(rng.integers(5, 30))
        o = oracle.step(cfg, st, steps, ticks, act, k)
        child.step(act, k)
        obs, rew, _, why = child.get_obs()
        _check(("fork", level, call), cfg, child.get_state(), (obs, rew, why) + child.get_counters(), (st, o[0], o[1], o[3], steps, ticks))
    parent.close()
    child.close()


# --------------------------------------------------------------------------------------------- what was covered
def test_zz_coverage_table(capsys):
    """Prints field -> forms it was varied on, and the worst error per quantity.  When the whole module has run, every physical
    field must have been varied both with all the others and alone."""
    with capsys.disabled():
        print("\nfield              forms it was varied on (all: every constant drawn at once; one: this field alone; done / reset / sampler)")
        for name in CS.physical_fields():
            labels = sorted(COVER.get(name, ()))
            print("%-18s %3d  %s" % (name, len(labels), "; ".join(labels[:6]) + (" ..." if len(labels) > 6 else "")))
        print("worst against the oracle: state group %.2e (< 1e-11), battery %.2e W s (< 1e-7), observation %.2e (< 1e-11), reward %.2e (< 1e-12)"
              % (WORST["state"], WORST["charge"], WORST["obs"], WORST["reward"]))
        print("BSK_DONE_ORBIT ties excused: %d of %d spacecraft-steps (%.4f %%)" % (WORST["orbit_ties"], WORST["envs"], 100.0 * WORST["orbit_ties"] / max(WORST["envs"], 1)))
    whole = len([r for r in RAN if r[0] == "all"]) == len(KI.STEPPED) and len([r for r in RAN if r[0] == "one"]) == len(ONE)
    if whole:
        for name in CS.physical_fields():
            labels = COVER.get(name, ())
            assert any(l.startswith("all:") for l in labels) and any(l.startswith("one:") for l in labels), name
