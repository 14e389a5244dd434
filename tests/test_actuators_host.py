"""CPU: the casts of tests/_actuators.py are what they claim - proven with the oracle's branch masks alone.  These are conditions on
the casts, not measurements of a kernel (tests/test_gpu_actuators.py runs them on the GPU).

The oracle is compiled a second time into ``tmp_path`` with oracle/Makefile's flags plus -DORC_BRANCH_MASK: a uint32 per spacecraft
that ORs a bit for every branch of the actuator chain taken during the last ``orc_step``.  For every config the GPU module runs:

- both builds give bit-identical outputs over the whole schedule;
- every bit is set by at least 8 characters of each cast that carries it (the wheel cast: command and wheel-speed bits only);
- in ``sorted`` some wave has EVERY lane with: a wheel at rest, a wheel's sign change within the schedule, (desat cast) a thruster
  active in a stage, a burst ending inside a step; some wave has NO lane with a thruster active during a launch in which another has;
  in ``mixed`` every wave holds lanes with and without it in the same launch;
- (desat cast) the ``t0`` slot under nav_lag = 1 requests nothing at its t = 0 tick, the K = 3 launch holds no FSW tick for it, the
  masked reset falls inside a running burst, and the burst limits 0, 12 (a stretched pulse) and 20 are latched;
- the either-way rule (``_actuators.kept``) leaves out at most 2 % of the characters and keeps 12 of 16 (48 of 64) in every slot.

The table of characters per bit and slot and the share left out are printed."""
import numpy as np
import pytest

import _actuators as A
from oracle import oracle


@pytest.fixture(scope="module")
def masklib(tmp_path_factory):
    return oracle.build_branch_mask(tmp_path_factory.mktemp("oracle_branch_mask"))


def test_default_build_has_no_branch_masks(masklib):
    assert not hasattr(oracle.load(), "orc_branch_mask") and hasattr(masklib, "orc_branch_mask")


def _configs(kind):
    forms = A.WHEEL_FORMS if kind == "wheel" else A.DESAT_FORMS
    seen, out = set(), []
    for form in forms:
        grav, n_rw, level, diag, _, _, _, nav, _ = forms[form]
        key = (grav, n_rw, "bare" if level == "ldss" else level, diag, nav)
        if key not in seen:
            seen.add(key)
            out.append(form)
    return out


@pytest.mark.parametrize("kind,form", [("wheel", f) for f in _configs("wheel")] + [("desat", f) for f in _configs("desat")])
def test_cast_takes_every_branch_where_the_layouts_need_it(kind, form, masklib, capsys):
    cfg, cast, _ = A.cast_for(kind, form)
    with capsys.disabled():
        runs, _ = A.prove(cast, masklib)
        report = {}
        ok = A.kept(cast, [{k: v for k, v in r.items() if k != "mask"} for r in runs], report)
        share = A.check_cap(cast, ok)
        print("either-way rule: %.2f %% of %d characters left out (%s); under the 1e-13 scaling the oracle moves by %.2f of a GPU bound, "
              "its sign-independent part by %.4f" % (100.0 * share, cast.M, {s: int((~ok[cast.where(s)]).sum()) for s in cast.slots if (~ok[cast.where(s)]).any()},
                                                      report["plain"], report["symmetric"]))
    lay = cast.layouts()
    assert sorted(lay["sorted"]) == list(range(cast.M)) and sorted(lay["mixed"]) == list(range(cast.M))
    assert 192 <= cast.M <= 768 and lay["embedded"].size == A.N_EMBEDDED and (lay["embedded"][:A.OFFSET] < 0).all()
    assert sum(A.KS) < 200 and len(A.KS) == 12 and max(A.KS) >= 60 and 3 in A.KS and 1 in A.KS


def test_either_way_rule_sees_a_character_on_an_edge():
    """A character moved ONTO an edge is left out, and only that one: a ``dead`` character whose largest command sits on u_min to the
    last bit that bisection reaches (everything about it is at rest, so the FSW tick of the first launch sees its initial state) -
    one scaled run commands u_min where the other commands zero."""
    cfg, cast, _ = A.cast_for("wheel", "bare-diag/nav0")
    saved = cast.state
    try:
        cast.state = saved.copy()
        c = int(cast.where("dead")[1])
        assert not cast.reset_mask[c]
        x, lo, hi = cast.state[:12 + cfg.n_rw, c].copy(), 1e-7, 1e-4
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            x[6:9] = np.array(list(cfg.sigma_R0N)) + mid * np.array([0.0, 1.0, 0.0])
            dead = np.abs(oracle.fsw(cfg, x, 1)[1]).max() == 0.0
            lo, hi = (mid, hi) if dead else (lo, mid)
        assert 1e-7 < lo < hi < 1e-4
        cast.state[6:9, c] = np.array(list(cfg.sigma_R0N)) + hi * np.array([0.0, 1.0, 0.0])
        ok = A.kept(cast)
        assert not ok[c] and ok.sum() == cast.M - 1, (ok[c], int((~ok).sum()))
    finally:
        cast.state = saved
