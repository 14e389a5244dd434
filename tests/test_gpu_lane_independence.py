"""GPU: a spacecraft's outputs are a function of its own state, counters, action and the config - bit for bit - whichever 63 others
share its wave, in every step-kernel form.

The step kernels cooperate across a wave: ballots choose one instantiation of the integrator step for the whole wave (drag, thruster
burst, the density guard, the t = 0 FSW tick), partially eclipsed ticks go through a per-wave queue that any lane may drain and that
is evaluated in place beyond its capacity, the wave-split forms exchange through LDS, and csrc/bsk_kernels.hip is compiled with
-ffp-contract=fast, under which two inlined copies of one function may round differently.  A test that compares two forms on the SAME
layout cannot see a dependence on neighbours, and the oracle bounds are 4 - 5 orders above one differently contracted multiply-add.
Here the same 192 characters (tests/_crowd.py: every regime, proven present by the oracle in tests/test_crowd_host.py) run in four
layouts - ``mixed`` (every wave holds every regime), ``sorted`` (the wave-uniform branches go the other way), ``embedded`` (other wave
and workgroup partners, a ragged tail) and ``solo`` (alone in an n = 1 handle) - through 14 launches (12 of one sub-step, a masked
host reset after the fourth, then 23 and 48 sub-steps):

(a) everything a launch leaves behind for a character is the same bits in all four: state rows, counters, observation, reward,
    reason, done byte and done-mask bit, the running / terminal returns and lengths, the row-major observation - no tolerance;
(b) ``mixed`` against ``oracle.step`` at the bounds of tests/test_gpu_config_space.py: _check (1e-11 per state group and observation,
    1e-12 reward, 1e-7 W s charge, reasons and counters exact), so the suite is never compared only with itself;
(c) device auto-reset from a ONE-slot pool (the slot rule then does not read the env index) with max_length = 3: restarts fall on
    different launches / history rows, each puts a t = 0 lane beside running ones; (a) with terminal observations and episode counts;
(d) the batch-wide ``static_charge`` shortcut (bare levels: withdrawn by one empty battery in the batch): a second ``mixed`` batch in
    which the empty batteries are charged - every OTHER character the same bits.

Every form tests/test_gpu_kernel_info.py: STEPPED pins, the halves form (one-sub-step launches) and the fused rollout kernel (every
history row); ``kernel_info()["name"]`` is asserted after every launch of every handle.  The last test prints the worst oracle error
per quantity.

FOUND with this module: every full-scenario form (single, general hub, pair, three-wave, generic facets, harmonics, and the scenario
kernel under device auto-reset) gave a spacecraft other low bits in ``sorted`` than in ``mixed`` from the first launch of more than one
sub-step on (the 23-sub-step launch; 120 - 140 of the 192 characters) - the third-body and density anchors sat at chunk heads cut by
the neighbours' FSW phases.  Fixed in csrc/bsk_kernels.hip (``since``).  The bare and power levels, the halves form and the rollout
kernel never differed.

Wall time on an MI355X: 6 s for the module's 30 tests once the session is up; no case above 0.5 s."""
import time

import numpy as np
import pytest

import _crowd as C
import test_gpu_kernel_info as KI
from basilisk_env_amd._lib import FLAG_AUTO_RESET, FLAG_EPISODE_STATS, FLAG_OBS_ROWMAJOR, FLAG_POWER, GRAV_PM, GRAV_PM_J2, T_CHARGE
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from helpers import max_group_err
from test_gpu_config_space import _propagator

pytestmark = pytest.mark.gpu

WORST = {"state": 0.0, "charge": 0.0, "obs": 0.0, "reward": 0.0, "spacecraft-steps": 0}
RAN = {}                       # form -> kernel names it ran under
LAYOUTS = ("mixed", "sorted", "embedded", "solo")


def _view(prop, views, key):
    import torch
    return torch.as_tensor(views[key], device="cuda").cpu().numpy()


def _snapshot(prop, pooled):
    """Everything a launch leaves behind, env on the last axis"""
    n = prop.n_envs
    steps, ticks = prop.get_counters()
    obs, rew, done, why = prop.get_obs()
    views = prop.device_views()
    words = _view(prop, views, "done_mask").view("<u8")
    e = np.arange(n)
    snap = {"state": prop.get_state(), "steps": steps, "ticks": ticks, "obs": obs, "reward": rew, "done": done, "reason": why,
            "mask_bit": ((words[e // 64] >> (e % 64).astype(np.uint64)) & np.uint64(1)).astype(np.uint8),
            "episode_return": _view(prop, views, "episode_return"), "terminal_return": _view(prop, views, "terminal_return"),
            "terminal_length": _view(prop, views, "terminal_length"), "done_byte": _view(prop, views, "done").astype(np.uint8),
            "obs_rowmajor": np.ascontiguousarray(_view(prop, views, "obs_rowmajor").T)}
    assert np.array_equal(np.asarray(prop.get_obs_rowmajor()[0]).T, snap["obs_rowmajor"])
    if pooled:
        tob, eps = prop.get_terminal_obs()
        snap["terminal_obs"] = np.where(done[None, :], tob, 0.0)           # (valid where the last step reported done)
        snap["episodes"] = eps
    return snap


def _handle(cfg, cast, n, sw, halves, pool):
    pair, tri, sh_form = sw
    prop = _propagator(cfg, n, pair, tri, sh_form, cast.sh)
    if halves:
        prop.set_halves_form(True)
    if pool is not None:
        prop.set_ic_pool(pool)
    return prop


def _run(cfg, cast, layout, sw, names, halves=False, pool=None, rollout=False, charged=None):
    """One layout through the schedule -> per launch {quantity: (..., M) array}, have (M,) bool.  ``names``: the kernel name each
    launch must report, by its sub-step count.  ``rollout``: the launches of one sub-step as two ``bsk_step_n`` calls (4 and 8 env
    steps, around the reset), the others as calls of one env step; the history rows join the quantities."""
    handles = cast.layouts()[layout]
    have = np.zeros(C.M, bool)
    calls = [(0, 4), (4, 12), (12, 13), (13, 14)] if rollout else [(c, c + 1) for c in range(len(C.KS))]
    out = [dict() for _ in calls]
    for n, index in handles:
        prop = _handle(cfg, cast, n, sw, halves, pool)
        st, steps, ticks = cast.batch(index, charged)
        prop.reset(st)
        prop.set_counters(steps, ticks)
        mine = index >= 0
        have[index[mine]] = True
        for ci, (lo, hi) in enumerate(calls):
            if lo == C.RESET_BEFORE:
                prop.reset(*cast.batch_reset(index))
            k = C.KS[lo]
            if rollout:
                acts = np.stack([cast.batch_actions(index, c) for c in range(lo, hi)])
                ho, hr, hw = prop.rollout(hi - lo, k, actions=acts)
            else:
                prop.step(cast.batch_actions(index, lo), k)
            snap = _snapshot(prop, pool is not None)
            if rollout:
                snap.update({"hist_obs": np.ascontiguousarray(ho.reshape(-1, n)), "hist_reward": hr, "hist_reason": hw})
            name = prop.kernel_info()["name"]
            assert name == names[k], (layout, n, lo, k, name, names[k])
            RAN.setdefault(names[max(names)], set()).add(name)
            for key, val in snap.items():
                full = out[ci].setdefault(key, np.zeros(val.shape[:-1] + (C.M,), val.dtype))
                full[..., index[mine]] = val[..., mine]
        prop.close()
    return out, have


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _assert_same(cast, form, runs, skip=None):
    """(a): every layout of ``runs`` {layout: (per launch quantities, have)} against the first, bit for bit"""
    base_name = next(iter(runs))
    base, _ = runs[base_name]
    for name, (got, have) in runs.items():
        if name == base_name:
            continue
        who = have if skip is None else have & ~skip
        for ci, (g, b) in enumerate(zip(got, base)):
            for key in b:
                x, y = _bits(g[key])[..., who], _bits(b[key])[..., who]
                if np.array_equal(x, y):
                    continue
                bad = np.argwhere(x != y)[0]
                c = int(np.flatnonzero(who)[bad[-1]])
                row = tuple(int(v) for v in bad[:-1])
                raise AssertionError("%s: character %d (%s) differs between layouts %r and %r after call %d in %s%s: %r against %r (%d characters differ)"
                                     % (form, c, cast.slot[c], name, base_name, ci, key, list(row), g[key][row + (c,)], b[key][row + (c,)],
                                        int(np.unique(np.argwhere(x != y)[:, -1]).size)))


def _check_oracle(form, cfg, cast, got, rollout=False):
    """(b): the mixed layout against the oracle (tests/test_gpu_config_space.py: _check, without the r_min tie rule - the cast keeps
    1e-9 away from r_min)"""
    ref = cast.run_oracle()                                       # in the cast's own order, as ``got`` is
    n_rw = cfg.n_rw
    groups = [(0, 4), (4, 12), (12, 13), (13, 14)] if rollout else [(c, c + 1) for c in range(len(C.KS))]
    for ci, (lo, hi) in enumerate(groups):
        g, (st, obs, rew, why, steps, ticks, _, _) = got[ci], ref[hi - 1]
        tag = (form, "call", ci)
        errs = max_group_err(g["state"], st, n_rw)
        WORST["state"] = max(WORST["state"], max(errs.values()))
        assert max(errs.values()) < 1e-11, (tag, errs)
        if cfg.flags & FLAG_POWER:
            dq = float(np.abs(g["state"][12 + n_rw + T_CHARGE] - st[12 + n_rw + T_CHARGE]).max())
            WORST["charge"] = max(WORST["charge"], dq)
            assert dq < 1e-7, (tag, dq)
        rows = [(g["obs"], g["reward"], g["reason"], obs, rew, why)]
        if rollout:
            ho = g["hist_obs"].reshape(hi - lo, 5, C.M)
            rows = [(ho[t], g["hist_reward"][t], g["hist_reason"][t], ref[lo + t][1], ref[lo + t][2], ref[lo + t][3]) for t in range(hi - lo)]
        for go, gr, gw, o, r, w in rows:
            eo, er = float(np.abs(go - o).max()), float(np.abs(gr - r).max())
            WORST["obs"], WORST["reward"] = max(WORST["obs"], eo), max(WORST["reward"], er)
            assert eo < 1e-11, (tag, eo, np.abs(go - o).max(axis=1))
            assert er < 1e-12, (tag, er)
            assert np.array_equal(gw, w), (tag, np.flatnonzero(gw != w)[:8])
        assert np.array_equal(g["steps"], steps) and np.array_equal(g["ticks"], ticks), tag
        assert np.array_equal(g["done"], why != 0) and np.array_equal(g["mask_bit"], (why != 0).astype(np.uint8)), tag
        WORST["spacecraft-steps"] += C.M * (hi - lo)


def _timed(t0, what):
    dt = time.time() - t0
    if dt > 5.0:
        print("\n[lane independence] %s took %.1f s" % (what, dt))


def _cast(grav, n_rw, level, diag, flags=0, max_length=None):
    cfg = C.crowd_config(KI.config(grav, n_rw, level, diag), level)
    cfg.flags |= FLAG_EPISODE_STATS | FLAG_OBS_ROWMAJOR | flags
    if max_length:
        cfg.max_length = max_length
    from basilisk_env_amd._lib import GRAV_SH
    from helpers import visible_sh_coefficients
    sh = visible_sh_coefficients(cfg.sh_degree, seed=3) if grav == GRAV_SH else (None, None)
    return cfg, C.Cast(cfg, level, sh)


def _charged(cast):
    return np.isin(cast.slot, ("battery", "both"))


# ------------------------------------------------------------------------------------------------ (a), (b), (d): every pinned form
@pytest.mark.parametrize("case", range(len(KI.STEPPED)), ids=[w[0] for _, w in KI.STEPPED])
def test_every_pinned_form_gives_a_character_the_same_bits_in_every_layout(case, capsys):
    t0 = time.time()
    (grav, n_rw, level, diag, pair, tri, sh_form), (want, _, _) = KI.STEPPED[case]
    cfg, cast = _cast(grav, n_rw, level, diag)
    names = {1: want, 23: want, 48: want}
    runs = {name: _run(cfg, cast, name, (pair, tri, sh_form), names) for name in LAYOUTS}
    _check_oracle(want, cfg, cast, runs["mixed"][0])
    _assert_same(cast, want, runs)
    if level in ("bare", "ldss"):                                  # (d): the empty batteries charged - the others must not notice
        charged = _run(cfg, cast, "mixed", (pair, tri, sh_form), names, charged=_charged(cast))
        _assert_same(cast, want + " (static_charge)", {"mixed": runs["mixed"], "mixed, every battery charged": charged}, skip=_charged(cast))
    with capsys.disabled():
        _timed(t0, want)


HALVES = [(GRAV_PM_J2, 4, True), (GRAV_PM, 3, False)]


@pytest.mark.parametrize("grav,n_rw,diag", HALVES)
def test_halves_form_gives_a_character_the_same_bits_in_every_layout(grav, n_rw, diag, capsys):
    """The one-sub-step launches in the halves form (the translational wave's 'below r_min' ballot and its r, v hand-over travel
    through LDS), the two long launches in the single-wave form of the same handles."""
    t0 = time.time()
    cfg, cast = _cast(grav, n_rw, "bare", diag)
    single = "step_kernel<%s,%d,%s>" % ({GRAV_PM: "PM", GRAV_PM_J2: "PM_J2"}[grav], n_rw, "diag" if diag else "full")
    names = {1: single[:-1] + ",halves>", 23: single, 48: single}
    runs = {name: _run(cfg, cast, name, ("0", "0", None), names, halves=True) for name in LAYOUTS}
    _check_oracle(names[1], cfg, cast, runs["mixed"][0])
    _assert_same(cast, names[1], runs)
    charged = _run(cfg, cast, "mixed", ("0", "0", None), names, halves=True, charged=_charged(cast))
    _assert_same(cast, names[1] + " (static_charge)", {"mixed": runs["mixed"], "mixed, every battery charged": charged}, skip=_charged(cast))
    with capsys.disabled():
        _timed(t0, names[1])


@pytest.mark.parametrize("grav,n_rw,diag", HALVES)
def test_rollout_kernel_gives_a_character_the_same_rows_in_every_layout(grav, n_rw, diag, capsys):
    """``bsk_step_n`` with per-step actions: 4 and 8 env steps of one sub-step in one launch each (the reset between them), then one
    env step of 23 and one of 48 - every history row, and what the handle holds after each launch."""
    t0 = time.time()
    cfg, cast = _cast(grav, n_rw, "bare", diag)
    want = "rollout_kernel<%s,%d,%s,actions>" % ({GRAV_PM: "PM", GRAV_PM_J2: "PM_J2"}[grav], n_rw, "diag" if diag else "full")
    names = {1: want, 23: want, 48: want}
    runs = {name: _run(cfg, cast, name, ("0", "0", None), names, rollout=True) for name in LAYOUTS}
    _check_oracle(want, cfg, cast, runs["mixed"][0], rollout=True)
    _assert_same(cast, want, runs)
    with capsys.disabled():
        _timed(t0, want)


# ------------------------------------------------------------------------------------------------ (c): device auto-reset
@pytest.mark.parametrize("grav,n_rw,level,rollout", [(GRAV_PM, 4, "bare", False), (GRAV_PM_J2, 3, "full", False), (GRAV_PM_J2, 4, "bare", True)],
                         ids=["bare", "scenario", "rollout"])
def test_device_auto_reset_from_a_one_slot_pool(grav, n_rw, level, rollout, capsys):
    t0 = time.time()
    cfg, cast = _cast(grav, n_rw, level, True, flags=FLAG_AUTO_RESET, max_length=3)
    g = {GRAV_PM: "PM", GRAV_PM_J2: "PM_J2"}[grav]
    want = ("rollout_kernel<%s,%d,diag,actions>" % (g, n_rw)) if rollout else "step_kernel<%s,%d,diag%s>" % (g, n_rw, ",scenario" if level == "full" else "")
    names = {1: want, 23: want, 48: want}
    pool = sample_ic_batch(1, n_rw, seed=77)
    runs = {name: _run(cfg, cast, name, ("0", "0", None), names, pool=pool, rollout=rollout) for name in LAYOUTS}
    _assert_same(cast, want + " (auto-reset)", runs)
    got = runs["mixed"][0]
    episodes = got[-1]["episodes"]
    ended = np.concatenate([g_["hist_reason"] for g_ in got]) != 0 if rollout else np.array([g_["done"] for g_ in got])      # (env steps, M)
    firsts = set(np.argmax(ended, axis=0)[ended.any(axis=0)].tolist())
    assert (episodes >= 2).sum() > C.M // 2 and len(firsts) >= 3, (episodes.min(), episodes.max(), sorted(firsts))   # restarts, on different steps
    # every wave of mixed has restarted lanes (t = 0 at the next env step) beside running ones, at the env steps of one sub-step
    index = cast.layouts()["mixed"][0][1]
    for w in range(0, C.M, 64):
        e = ended[:12, index[w:w + 64]]
        assert (e.any(axis=1) & ~e.all(axis=1)).any(), w
    with capsys.disabled():
        _timed(t0, want + " (auto-reset)")


def test_zz_worst_oracle_error_and_forms(capsys):
    with capsys.disabled():
        print("\n[lane independence] mixed layout against the oracle over %d spacecraft-steps: state group %.2e (< 1e-11), battery %.2e W s (< 1e-7), "
              "observation %.2e (< 1e-11), reward %.2e (< 1e-12)" % (WORST["spacecraft-steps"], WORST["state"], WORST["charge"], WORST["obs"], WORST["reward"]))
        for form in sorted(RAN):
            print("  ran: %s" % ", ".join(sorted(RAN[form])))
