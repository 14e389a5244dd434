"""GPU: the data-dependent branches of the attitude guidance chain - hillPoint | inertial3D -> attTrackingError - and the shadow-set
switch against the CPU oracle, branch by branch, in every kernel form that carries the code.

The cast of tests/_guidance.py (every branch proven taken, with the oracle's branch masks, in tests/test_guidance_host.py: the
three reference choices with whole waves on the navigation message nobody has written, the four Sheppard cases of ``c2mrp`` with and
without the b0 < 0 flip, whole and mixed waves inside ``submrp``'s guard |den| < 0.1 and just outside it, the inner-set map, the
shadow-set switch inside launches of every K) runs through 12 launches (181 ticks) in three layouts - ``sorted`` (whole waves of one
slot), ``mixed`` and ``embedded`` (n = 333).  The first launch (K = 16: the pair and three-wave forms where they are built) and the
K = 1 launch after the masked host reset (the halves form) run the FSW tick on the states as constructed.

After EVERY launch of EVERY layout, for the characters the either-way rule keeps, against ``oracle.step``: state groups
(helpers.max_group_err) and observation < 1e-11, reward < 1e-12, UCMD, UPEND and SBR within 1e-11, reason, counters and the thruster
schedule exact - the bounds of tests/test_gpu_actuators.py.  Across layouts every kept character gives the same bits, and so does
every ``tie`` character, kept or not (lane independence needs no oracle).  ``kernel_info()["name"]`` is asserted after every launch.

Forms: the rows of ``_actuators.WHEEL_FORMS`` (single-wave bare with diagonal and general hub, lds-scratch, the fused rollout kernel,
power single-wave and pair - each under nav_lag 0 and 1 - and the halves form under nav_lag 1) and ``DESAT_FORMS`` (scenario single-wave
with diagonal and general hub, pair, three-wave, generic facets, harmonics SH/dpp and SH/dpp2 at degree 8), and the bare form without
wheels (guidance still feeds obs[0]; ``control``'s loop is empty).  Once each: the cast forked into a second handle right after the
launch in which a whole wave took the guard, continuing bit for bit; ``bsk_step_n``'s fallback against single launches.

The last test prints the worst error per quantity, the characters left out and the module's wall time.  On an MI355X: state group
3.5e-14, observation 6.7e-14, reward 1.1e-18, SBR 1.0e-15, UCMD / UPEND 6.9e-15, THR_REM 3.3e-14 s; none of the 5 520 characters
outside ``tie`` of the 15 casts left out, and all 360 ``tie`` characters kept by the rule as this module applies it (with the guidance
bits compared too, tests/test_guidance_host.py keeps 21 - 24 of each cast's 24); 2.4 s for the module's 24 tests once the session
is up, no case above 0.4 s.  The unmutated kernels passed at the first run: no defect found in them, nor in the oracle (50 digits:
``c2mrp`` 2.3e-16, ``submrp`` 4.0e-16 of a bound of 1e-13).

THAT THE TESTS CAN FAIL - one change each in a copy of csrc/bsk_device.hpp, one build each (all seven built), the cases of
test_guidance_cast_matches_the_oracle_in_every_layout (21) that turned red, and what tests/test_gpu_lane_independence.py,
test_gpu_fuzz.py and test_gpu_parity.py (153 tests) see of it:
  1 s1 / s2 swapped in c2mrp's case-3 numerators     all 21, the fork        older: 62 fuzz seeds, lane independence 26, parity 41
  2 the b0 < 0 flip dropped                          NONE                    older: none
  3 submrp's guard never taken                       20 (all with wheels), the fork        older: parity's long-horizon test only
  4 submrp's inner-set map dropped                   all 21, the fork        older: 65 fuzz seeds, lane independence 26, parity 47
  5 the final zeroing of hill_point<true> dropped    the 14 under nav_lag = 1, the fork    older: 29 fuzz seeds, lane independence 23, parity 26
  6 no shadow switch in the halves form's attitude   halves/nav1             older: lane independence's two halves cases
  7 the sign of ddfdt2 flipped                       20 (all with wheels), the fork        older: 37 fuzz seeds, lane independence 23, parity 29
2 is an equivalent mutant, not a hole in the cast: the flip only chooses the MRP set of sigma_RN, which feeds ``submrp`` alone, and
``submrp``'s result does not depend on that set (tests/test_guidance_host.py: test_the_flip_changes_no_tracking_error holds the two
to 1e-13 on the flip slots, and every character of those slots is proven to take the flip in the first launch).  3 passed the cast as
first built - |den| from 1.2e-3 up, where the unguarded formula errs by 1e-16 / den in the length of the same attitude - and fails
since every third and fourth ``guard`` character is converged on the other MRP set (|den| = 1e-15 .. 1e-9): omega and Omega off by
1e-9.  Without wheels no FSW tick runs, so the guard is reached on the inner set only (|den| >= 1.2e-2) and domega_RN_B is unused:
3 and 7 pass there.  Unlike the actuator chain's, none of these changes was invisible to the older modules except 2; what this
module adds is that each is seen in EVERY form, on proven branches (1, 4, 5, 7 fail the older modules on whichever seeds reach them)."""
import time

import numpy as np
import pytest

import _actuators as A
import _guidance as G
from basilisk_env_amd import _lib
from basilisk_env_amd._lib import FLAG_EPISODE_STATS, FLAG_OBS_ROWMAJOR
from helpers import max_group_err
from test_gpu_config_space import _propagator
from test_gpu_lane_independence import _assert_same, _snapshot

pytestmark = pytest.mark.gpu

LAYOUTS = ("sorted", "mixed", "embedded")
WORST = {"state": 0.0, "obs": 0.0, "reward": 0.0, "thr_rem": 0.0, "command": 0.0, "sbr": 0.0, "spacecraft-steps": 0, "left out": 0, "characters": 0,
         "tie kept": 0, "tie": 0}
RAN = {}
T_START = [None]
_REF = {}


def _reference(form):
    """(cfg, cast, row, oracle runs, kept) - the oracle's side, computed once per cast and shared (the default build only: the
    guidance bits of the either-way rule are tests/test_guidance_host.py's)"""
    cfg, cast, row = G.cast_for(form)
    cfg.flags |= FLAG_EPISODE_STATS | FLAG_OBS_ROWMAJOR
    if id(cast) not in _REF:
        ref = cast.run_oracle()
        ok = A.kept(cast, ref, sbr=True)
        A.check_cap(cast, ok, G.EXEMPT)
        _REF[id(cast)] = (ref, ok)
        tie = cast.slot == "tie"
        WORST["left out"] += int((~ok[~tie]).sum())
        WORST["characters"] += int((~tie).sum())
        WORST["tie kept"] += int(ok[tie].sum())
        WORST["tie"] += int(tie.sum())
    return (cfg, cast, row) + _REF[id(cast)]


def _groups(how):
    """the launches as calls: one each, or (rollout) runs of equal K that the reset does not split, as rows of one ``bsk_step_n``"""
    if how != "rollout":
        return [(c, c + 1) for c in range(len(G.KS))]
    out, lo = [], 0
    for c in range(1, len(G.KS) + 1):
        if c == len(G.KS) or G.KS[c] != G.KS[lo] or c == G.RESET_BEFORE:
            out.append((lo, c))
            lo = c
    return out


def _reset(prop, cast, index):
    """the masked host reset: the reset characters restart from their spare states with their own counters"""
    prop.reset(*cast.batch_reset(index))
    prop.set_counters(*cast.batch_reset_counters(index, *prop.get_counters()))


def _run(cfg, cast, row, layout, via_step_n=False):
    """One layout through the schedule -> per call {quantity: (..., M) array}, have (M,) bool"""
    _, _, _, _, pair, tri, sh_form, _, how = row
    names = A.names_for(cfg, row)
    index = cast.layouts()[layout]
    n, mine = index.size, index >= 0
    have = np.zeros(cast.M, bool)
    have[index[mine]] = True
    calls = _groups("rollout" if via_step_n else how)
    out = [dict() for _ in calls]
    prop = _propagator(cfg, n, pair, tri, sh_form, cast.sh)
    try:
        if how == "halves":
            prop.set_halves_form(True)
        st, steps, ticks = cast.batch(index)
        prop.reset(st)
        prop.set_counters(steps, ticks)
        for ci, (lo, hi) in enumerate(calls):
            if lo == G.RESET_BEFORE:
                _reset(prop, cast, index)
            k = G.KS[lo]
            hist = None
            if how == "rollout" or via_step_n:
                hist = prop.rollout(hi - lo, k, actions=np.stack([cast.batch_actions(index, c) for c in range(lo, hi)]))
            else:
                prop.step(cast.batch_actions(index, lo), k)
            snap = _snapshot(prop, False)
            if hist is not None:
                snap.update({"hist_obs": np.ascontiguousarray(hist[0].reshape(-1, n)), "hist_reward": hist[1], "hist_reason": hist[2]})
            name = prop.kernel_info()["name"]
            assert name == names[k], (layout, n, lo, k, name, names[k])
            RAN.setdefault(name, 0)
            RAN[name] += 1
            for key, val in snap.items():
                full = out[ci].setdefault(key, np.zeros(val.shape[:-1] + (cast.M,), val.dtype))
                full[..., index[mine]] = val[..., mine]
    finally:
        prop.close()
    return out, have


def _check_oracle(tag, cfg, cast, got, have, ref, ok, how="step"):
    """every call of one layout against the oracle, on the kept characters the layout holds"""
    n_rw, who = cfg.n_rw, have & ok
    tail = _lib.NF_BASE + n_rw
    rem = slice(tail + _lib.T_THR_REM, tail + _lib.T_THR_REM + 8)
    ints = slice(tail + _lib.T_THR_LIM, tail + _lib.T_THR_CNT + 1)
    for ci, (lo, hi) in enumerate(_groups(how)):
        g, r = got[ci], ref[hi - 1]
        t = tag + ("call", ci, "K", G.KS[lo])
        s, o = g["state"][:, who], r["state"][:, who]
        errs = max_group_err(s, o, n_rw)
        WORST["state"] = max(WORST["state"], max(errs.values()))
        assert max(errs.values()) < 1e-11, (t, errs)
        e_rem = float(np.abs(s[rem] - o[rem]).max())
        WORST["thr_rem"] = max(WORST["thr_rem"], e_rem)
        assert e_rem < 1e-12, (t, e_rem)
        assert np.array_equal(s[ints], o[ints]), (t, "THR_LIM / THR_T0 / THR_CNT", np.flatnonzero(who)[np.flatnonzero((s[ints] != o[ints]).any(axis=0))][:8])
        e_sbr = np.abs(s[tail + _lib.T_SBR] - o[tail + _lib.T_SBR])
        WORST["sbr"] = max(WORST["sbr"], float(e_sbr.max()))
        assert e_sbr.max() < 1e-11, (t, "SBR", float(e_sbr.max()), cast.slot[np.flatnonzero(who)[int(e_sbr.argmax())]])
        for f in (_lib.T_UCMD, _lib.T_UPEND):
            a, b = s[tail + f:tail + f + 4], o[tail + f:tail + f + 4]
            e_cmd = float(np.abs(a - b).max())
            WORST["command"] = max(WORST["command"], e_cmd)
            assert e_cmd < 1e-11, (t, f, e_cmd, cast.slot[np.flatnonzero(who)[int(np.abs(a - b).max(axis=0).argmax())]])
            for edge in (0.0, cfg.u_max, -cfg.u_max):            # the clamp and the dead-band give the value itself, not one near it
                assert np.array_equal(a == edge, b == edge), (t, f, edge, np.flatnonzero(who)[np.flatnonzero(((a == edge) != (b == edge)).any(axis=0))][:8])
        rows = [(g["obs"], g["reward"], g["reason"], r)]
        if how == "rollout":
            ho = g["hist_obs"].reshape(hi - lo, 5, cast.M)
            rows = [(ho[i], g["hist_reward"][i], g["hist_reason"][i], ref[lo + i]) for i in range(hi - lo)]
        for go, gr, gw, rr in rows:
            eo, er = np.abs(go[:, who] - rr["obs"][:, who]), float(np.abs(gr[who] - rr["reward"][who]).max())
            WORST["obs"], WORST["reward"] = max(WORST["obs"], float(eo.max())), max(WORST["reward"], er)
            assert eo.max() < 1e-11, (t, float(eo.max()), eo.max(axis=1), cast.slot[np.flatnonzero(who)[int(eo.max(axis=0).argmax())]])
            assert er < 1e-12, (t, er)
            assert np.array_equal(gw[who], rr["reason"][who]), (t, "reason", np.flatnonzero(who)[np.flatnonzero(gw[who] != rr["reason"][who])][:8])
        assert np.array_equal(g["steps"][who], r["steps"][who]) and np.array_equal(g["ticks"][who], r["ticks"][who]), t
        assert np.array_equal(g["done"][who], r["reason"][who] != 0), t
        WORST["spacecraft-steps"] += int(who.sum()) * (hi - lo)


@pytest.mark.parametrize("form", list(G.FORMS))
def test_guidance_cast_matches_the_oracle_in_every_layout(form):
    if T_START[0] is None:
        T_START[0] = time.time()
    cfg, cast, row, ref, ok = _reference(form)
    how = row[-1]
    runs = {}
    for layout in LAYOUTS:
        runs[layout] = _run(cfg, cast, row, layout)
        _check_oracle((form, layout), cfg, cast, runs[layout][0], runs[layout][1], ref, ok, how)
    _assert_same(cast, "guidance cast, %s" % form, runs, skip=~ok & (cast.slot != "tie"))
    want = set(A.names_for(cfg, row).values())
    assert want <= set(RAN), want - set(RAN)


def test_cast_forked_after_the_guard_fired_continues_bit_for_bit():
    """``fork_from`` after the first launch, in which every lane of the first wave of ``sorted`` took ``submrp``'s guard (|den| < 0.1
    on the state the FSW tick saw): the copy runs the rest of the schedule (the masked reset included) to the same bits as its source."""
    cfg, cast, row, ref, ok = _reference("scenario-diag")
    index = cast.layouts()["sorted"]
    n = index.size
    first = index[:64]
    assert (cast.slot[first] == "guard").all()
    den = np.array([G.submrp_raw(cast.state[6:9, c], G.sigma_ref(cfg, cast.state[:, c], int(cast.actions[0, c])))[0] for c in first])
    assert (np.abs(den) < 0.1).all() and cfg.nav_lag == 1 and (cast.ticks[first] % cfg.fsw_every == cfg.fsw_every - 1).all()
    a, b = _propagator(cfg, n, "0", "0", None, cast.sh), _propagator(cfg, n, "0", "0", None, cast.sh)
    try:
        st, steps, ticks = cast.batch(index)
        a.reset(st)
        a.set_counters(steps, ticks)
        b.reset(cast.batch(cast.layouts()["mixed"])[0])               # (something else, to be overwritten)
        a.step(cast.batch_actions(index, 0), G.KS[0])
        b.fork_from(a, np.arange(n))
        for c in range(1, len(G.KS)):
            for p in (a, b):
                if c == G.RESET_BEFORE:
                    _reset(p, cast, index)
                p.step(cast.batch_actions(index, c), G.KS[c])
            sa, sb = _snapshot(a, False), _snapshot(b, False)
            for key in sa:
                assert np.array_equal(sa[key], sb[key], equal_nan=True), (c, key)
        last, r = sb["state"][:, np.argsort(index)][:, ok], ref[-1]["state"][:, ok]
        assert max(max_group_err(last, r, cfg.n_rw).values()) < 1e-11
    finally:
        a.close()
        b.close()


def test_step_n_fallback_equals_single_launches():
    """``bsk_step_n`` where no rollout kernel is built (the full scenario) falls back to single launches of the step kernel: the
    cast through the schedule as ``bsk_step_n`` rows and as ``bsk_step`` calls - the same bits, the step kernel's name."""
    cfg, cast, row, ref, ok = _reference("tri")
    single = _run(cfg, cast, row, "mixed")
    rows = _run(cfg, cast, row, "mixed", via_step_n=True)
    for ci, (lo, hi) in enumerate(_groups("rollout")):
        g, s = rows[0][ci], single[0][hi - 1]
        for key in s:
            assert np.array_equal(g[key], s[key], equal_nan=True), (ci, key)
        for i in range(hi - lo):
            assert np.array_equal(g["hist_reason"][i], single[0][lo + i]["reason"]) and np.array_equal(g["hist_reward"][i], single[0][lo + i]["reward"])
            assert np.array_equal(g["hist_obs"].reshape(hi - lo, 5, cast.M)[i], single[0][lo + i]["obs"])


def test_zz_worst_errors_and_wall_time(capsys):
    with capsys.disabled():
        print("\n[guidance] kept characters against the oracle over %d spacecraft-launches: state group %.2e (< 1e-11), observation %.2e (< 1e-11), "
              "reward %.2e (< 1e-12), SBR %.2e (< 1e-11), UCMD / UPEND %.2e (< 1e-11), THR_REM %.2e s (< 1e-12); %d of %d characters outside tie left "
              "out by the either-way rule, tie keeps %d of %d"
              % (WORST["spacecraft-steps"], WORST["state"], WORST["obs"], WORST["reward"], WORST["sbr"], WORST["command"], WORST["thr_rem"],
                 WORST["left out"], WORST["characters"], WORST["tie kept"], WORST["tie"]))
        for name in sorted(RAN):
            print("  ran: %-60s %4d launches" % (name, RAN[name]))
        if T_START[0] is not None:
            print("[guidance] module wall time %.1f s" % (time.time() - T_START[0]))
