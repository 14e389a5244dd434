"""GPU: the data-dependent branches of the wheel and thruster command chain against the CPU oracle, branch by branch, in every kernel
form that carries the code.

The casts of tests/_actuators.py (every branch proven taken, with the oracle's branch masks, in tests/test_actuators_host.py: the
u_max clamp and the u_min dead-band, a wheel at rest and at its zero crossing under the branch-free friction clamp(2^1000 Om, -fc, fc),
every branch of ``desat_tick``, waves with every, some and no lane inside a thruster burst) run through 12 launches (181 ticks, a
masked host reset after the third) in three layouts - ``sorted`` (whole waves of one slot), ``mixed`` and ``embedded`` (n = 333).

After EVERY launch of EVERY layout, for the characters the either-way rule keeps (``_actuators.kept``), against ``oracle.step``:
state groups (helpers.max_group_err) and observation < 1e-11, reward < 1e-12, THR_REM < 1e-12 s, reason, counters, THR_LIM, THR_T0 and
THR_CNT exact, UCMD and UPEND within 1e-11 and exactly 0 / +-u_max where the oracle's are (the bounds of tests/test_gpu_desat.py and
tests/test_gpu_fuzz.py).  Across layouts every kept character gives the same bits (tests/test_gpu_lane_independence.py: _assert_same).
``kernel_info()["name"]`` is asserted after every launch.

Wheel cast: single-wave bare (diagonal and general hub), lds-scratch, the halves form (its K = 1 launches), the fused rollout kernel
(``bsk_step_n`` rows), power single-wave and pair - each under nav_lag 0 and 1 (halves: 1).  Desat cast: scenario single-wave (diagonal
and general hub), pair, three-wave, generic facets, harmonics SH/dpp and SH/dpp2 at degree 8.  Once each: the desat cast forked
mid-burst into a second handle, which continues bit for bit; ``bsk_step_n``'s fallback against single launches; and the largest
stretched burst limit that fits its 16 bits (65535), next to a neighbour's in the same register.

The last test prints the worst error per quantity and the module's wall time.  On an MI355X: state group 2.2e-13, observation 7.0e-14,
reward 1.3e-18, THR_REM 1.7e-13 s, UCMD / UPEND 4.4e-14; none of the 3 744 characters of the 14 casts left out; 2 s for the module's 24
tests once the session is up, no case above 0.4 s.  The unmutated kernels passed at the first run: no defect found in them.

THAT THE TESTS CAN FAIL - one change each in a copy of csrc/bsk_device.hpp or csrc/bsk_kernels.hip, one build each, the tests that
turned red (and whether tests/test_gpu_desat.py, test_gpu_fuzz.py or test_gpu_lane_independence.py, 100 tests, see it too):
  1 friction as copysign(fc, Om) - a wheel at rest feels friction   every wheel and desat case, the fork (21)   older: none
  2 the dead-band test dropped                                      every wheel and desat case, the fork (21)   older: 7 fuzz seeds, the env test
  3 the thr_min_fire_time test dropped                              every desat case, the fork (8)              older: none
  4 fmax(on, thr_min_on_time) replaced by on                        every desat case, the fork, the limit (9)   older: none
  5 ev.thr_on from lane 0 instead of the ballot                     desat pair and tri - the forms that hold it  older: desat (3), fuzz seed 29,
                                                                                                                lane independence pair, tri (3)
  6 thr_cnt not reloaded (launches without a request store it back) every desat case, the limit (8)             older: test_desat_matches_oracle (2)
  7 the single-wave forms' burst decision (uni_any) from lane 0     every desat case, the fork (8)              older: desat (2), 11 fuzz seeds,
                                                                                                                lane independence (7)
1, 3 and 4 - friction at rest, the dropped and the stretched pulse - were seen by no test before this module."""
import time

import numpy as np
import pytest

import _actuators as A
from basilisk_env_amd import _lib
from basilisk_env_amd._lib import FLAG_DESAT, FLAG_EPISODE_STATS, FLAG_OBS_ROWMAJOR, FLAG_POWER, GRAV_PM_J2
from basilisk_env_amd.simulators.dynamics import BatchedPropagator, default_config
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from helpers import max_group_err
from oracle import oracle
from test_gpu_config_space import _propagator
from test_gpu_lane_independence import _assert_same, _snapshot

pytestmark = pytest.mark.gpu

LAYOUTS = ("sorted", "mixed", "embedded")
WORST = {"state": 0.0, "obs": 0.0, "reward": 0.0, "thr_rem": 0.0, "command": 0.0, "spacecraft-steps": 0, "left out": 0, "characters": 0}
RAN = {}
T_START = [None]
_REF = {}


def _reference(kind, form):
    """(cfg, cast, row, oracle runs, kept) - the oracle's side, computed once per cast and shared"""
    cfg, cast, row = A.cast_for(kind, form)
    cfg.flags |= FLAG_EPISODE_STATS | FLAG_OBS_ROWMAJOR
    if id(cast) not in _REF:
        ref = cast.run_oracle()
        ok = A.kept(cast, ref)
        A.check_cap(cast, ok)
        _REF[id(cast)] = (ref, ok)
        WORST["left out"] += int((~ok).sum())
        WORST["characters"] += cast.M
    return (cfg, cast, row) + _REF[id(cast)]


def _groups(how):
    """the launches as calls: one each, or (rollout) runs of equal K that the reset does not split, as rows of one ``bsk_step_n``"""
    if how != "rollout":
        return [(c, c + 1) for c in range(len(A.KS))]
    out, lo = [], 0
    for c in range(1, len(A.KS) + 1):
        if c == len(A.KS) or A.KS[c] != A.KS[lo] or c == A.RESET_BEFORE:
            out.append((lo, c))
            lo = c
    return out


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
            if lo == A.RESET_BEFORE:
                prop.reset(*cast.batch_reset(index))
            k = A.KS[lo]
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
        t = tag + ("call", ci, "K", A.KS[lo])
        s, o = g["state"][:, who], r["state"][:, who]
        errs = max_group_err(s, o, n_rw)
        WORST["state"] = max(WORST["state"], max(errs.values()))
        assert max(errs.values()) < 1e-11, (t, errs)
        e_rem = float(np.abs(s[rem] - o[rem]).max())
        WORST["thr_rem"] = max(WORST["thr_rem"], e_rem)
        assert e_rem < 1e-12, (t, e_rem)
        assert np.array_equal(s[ints], o[ints]), (t, "THR_LIM / THR_T0 / THR_CNT", np.flatnonzero(who)[np.flatnonzero((s[ints] != o[ints]).any(axis=0))][:8])
        for f in (_lib.T_UCMD, _lib.T_UPEND):
            a, b = s[tail + f:tail + f + n_rw], o[tail + f:tail + f + n_rw]
            e_cmd = float(np.abs(a - b).max())
            WORST["command"] = max(WORST["command"], e_cmd)
            assert e_cmd < 1e-11, (t, f, e_cmd)
            for edge in (0.0, cfg.u_max, -cfg.u_max):            # the clamp and the dead-band give the value itself, not one near it
                assert np.array_equal(a == edge, b == edge), (t, f, edge, np.flatnonzero(who)[np.flatnonzero(((a == edge) != (b == edge)).any(axis=0))][:8])
        rows = [(g["obs"], g["reward"], g["reason"], r)]
        if how == "rollout":
            ho = g["hist_obs"].reshape(hi - lo, 5, cast.M)
            rows = [(ho[i], g["hist_reward"][i], g["hist_reason"][i], ref[lo + i]) for i in range(hi - lo)]
        for go, gr, gw, rr in rows:
            eo, er = float(np.abs(go[:, who] - rr["obs"][:, who]).max()), float(np.abs(gr[who] - rr["reward"][who]).max())
            WORST["obs"], WORST["reward"] = max(WORST["obs"], eo), max(WORST["reward"], er)
            assert eo < 1e-11, (t, eo, np.abs(go[:, who] - rr["obs"][:, who]).max(axis=1))
            assert er < 1e-12, (t, er)
            assert np.array_equal(gw[who], rr["reason"][who]), (t, "reason", np.flatnonzero(who)[np.flatnonzero(gw[who] != rr["reason"][who])][:8])
        assert np.array_equal(g["steps"][who], r["steps"][who]) and np.array_equal(g["ticks"][who], r["ticks"][who]), t
        assert np.array_equal(g["done"][who], r["reason"][who] != 0), t
        WORST["spacecraft-steps"] += int(who.sum()) * (hi - lo)


def _case(kind, form):
    if T_START[0] is None:
        T_START[0] = time.time()
    cfg, cast, row, ref, ok = _reference(kind, form)
    how = row[-1]
    runs = {}
    for layout in LAYOUTS:
        runs[layout] = _run(cfg, cast, row, layout)
        _check_oracle((kind, form, layout), cfg, cast, runs[layout][0], runs[layout][1], ref, ok, how)
    _assert_same(cast, "%s cast, %s" % (kind, form), runs, skip=~ok)
    want = set(A.names_for(cfg, row).values())
    assert want <= set(RAN), want - set(RAN)


@pytest.mark.parametrize("form", list(A.WHEEL_FORMS))
def test_wheel_cast_matches_the_oracle_in_every_layout(form):
    _case("wheel", form)


@pytest.mark.parametrize("form", list(A.DESAT_FORMS))
def test_desat_cast_matches_the_oracle_in_every_layout(form):
    _case("desat", form)


def test_desat_cast_forked_mid_burst_continues_bit_for_bit():
    """``fork_from`` after the first launch, when every lane of the ``dump`` wave is inside a burst: the copy runs the rest of the schedule (the
    masked reset included) to the same bits as its source."""
    cfg, cast, row, ref, ok = _reference("desat", "scenario-diag")
    index = cast.layouts()["sorted"]
    n, tail = index.size, _lib.NF_BASE + cfg.n_rw
    a, b = _propagator(cfg, n, "0", "0", None, cast.sh), _propagator(cfg, n, "0", "0", None, cast.sh)
    try:
        st, steps, ticks = cast.batch(index)
        a.reset(st)
        a.set_counters(steps, ticks)
        b.reset(cast.batch(cast.layouts()["mixed"])[0])               # (something else, to be overwritten)
        a.step(cast.batch_actions(index, 0), A.KS[0])
        s, (_, tk) = a.get_state(), a.get_counters()
        lim = s[tail + _lib.T_THR_LIM:tail + _lib.T_THR_LIM + 8].max(axis=0)
        inside = (lim > 0) & (2 * (tk - s[tail + _lib.T_THR_T0]) <= lim)
        assert inside[:64].all() and (cast.slot[index[:64]] == "dump").all(), int(inside[:64].sum())       # mid-burst, a whole wave
        b.fork_from(a, np.arange(n))
        for c in range(1, len(A.KS)):
            for p in (a, b):
                if c == A.RESET_BEFORE:
                    p.reset(*cast.batch_reset(index))
                p.step(cast.batch_actions(index, c), A.KS[c])
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
    desat cast through the schedule as ``bsk_step_n`` rows and as ``bsk_step`` calls - the same bits, the step kernel's name."""
    cfg, cast, row, ref, ok = _reference("desat", "tri")
    single = _run(cfg, cast, row, "mixed")
    rows = _run(cfg, cast, row, "mixed", via_step_n=True)
    groups = _groups("rollout")
    for ci, (lo, hi) in enumerate(groups):
        g, s = rows[0][ci], single[0][hi - 1]
        for key in s:
            assert np.array_equal(g[key], s[key], equal_nan=True), (ci, key)
        for i in range(hi - lo):
            assert np.array_equal(g["hist_reason"][i], single[0][lo + i]["reason"]) and np.array_equal(g["hist_reward"][i], single[0][lo + i]["reward"])
            assert np.array_equal(g["hist_obs"].reshape(hi - lo, 5, cast.M)[i], single[0][lo + i]["obs"])


def test_largest_burst_limit_that_fits_is_exact():
    """floor(thr_min_on_time * 2 / dt) = 65535, one below what ``bsk_create`` refuses (tests/test_abi.py): with thr_min_fire_time = 0
    the thruster that owes nothing is stretched to it, next to neighbours with the full-period limit in the same 32-bit register -
    every limit equals the oracle's."""
    n, n_rw = 64, 4
    cfg = default_config(n_rw, GRAV_PM_J2)
    cfg.flags |= FLAG_POWER | FLAG_DESAT
    cfg.thr_min_fire_time, cfg.thr_min_on_time = 0.0, 3276.775
    assert np.floor(cfg.thr_min_on_time * (2.0 / cfg.dt)) == 65535.0
    ic = sample_ic_batch(n, n_rw, seed=12)
    ic[12:12 + n_rw] *= 2.5
    st, steps, ticks = ic.copy(), np.ones(n, np.int32), np.full(n, 5, np.int32)
    tail = _lib.NF_BASE + n_rw
    lims = slice(tail + _lib.T_THR_LIM, tail + _lib.T_THR_LIM + 8)
    prop = BatchedPropagator(cfg, n)
    try:
        prop.reset(ic)
        prop.set_counters(steps, ticks)
        act = np.full(n, 2, np.int32)
        for k in (10, 3):
            oracle.step(cfg, st, steps, ticks, act, k)
            prop.step(act, k)
            s = prop.get_state()
            assert np.array_equal(s[lims], st[lims]), k
            assert np.array_equal(s[tail + _lib.T_THR_T0], st[tail + _lib.T_THR_T0]) and np.array_equal(s[tail + _lib.T_THR_CNT], st[tail + _lib.T_THR_CNT])
            assert max(max_group_err(s, st, n_rw).values()) < 1e-11
        first = st[lims]
        assert (first == 65535.0).any(axis=0).all() and (first == 2.0 * cfg.fsw_every).any(axis=0).sum() > n // 2, np.unique(first)
        pairs = first.reshape(4, 2, n)                               # (register, half, spacecraft)
        assert ((pairs[:, 0] == 65535.0) & (pairs[:, 1] != 65535.0)).any() and ((pairs[:, 1] == 65535.0) & (pairs[:, 0] != 65535.0)).any()
    finally:
        prop.close()


def test_zz_worst_errors_and_wall_time(capsys):
    with capsys.disabled():
        print("\n[actuators] kept characters against the oracle over %d spacecraft-launches: state group %.2e (< 1e-11), observation %.2e (< 1e-11), "
              "reward %.2e (< 1e-12), THR_REM %.2e s (< 1e-12), UCMD / UPEND %.2e (< 1e-11); %d of %d characters left out by the either-way rule"
              % (WORST["spacecraft-steps"], WORST["state"], WORST["obs"], WORST["reward"], WORST["thr_rem"], WORST["command"], WORST["left out"], WORST["characters"]))
        for name in sorted(RAN):
            print("  ran: %-60s %4d launches" % (name, RAN[name]))
        if T_START[0] is not None:
            print("[actuators] module wall time %.1f s" % (time.time() - T_START[0]))
