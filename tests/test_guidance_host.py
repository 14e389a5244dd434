"""CPU: the cast of tests/_guidance.py is what it claims - proven with the oracle's branch masks - and the oracle's own ``c2mrp`` and
``submrp`` hold against 50 digits on everything the cast feeds them.  These are conditions on the cast and the oracle, not
measurements of a kernel (tests/test_gpu_guidance.py runs the cast on the GPU).

The oracle is compiled a second time into ``tmp_path`` with -DORC_BRANCH_MASK (tests/test_actuators_host.py); bits 19 .. 29 mark
the reference choice, the Sheppard case and the b0 < 0 flip, the guard and the inner-set map of ``submrp`` and the shadow-set switch
after an RK4 step, inside the functions themselves, whoever calls them.  For every config the GPU module runs:

- both builds give bit-identical outputs over the whole schedule;
- presence: every bit is taken by at least 8 kept characters of the slot that exists for it - in the first launch and again in the
  K = 1 launch after the masked reset, whose FSW ticks see the states as constructed; each ``case`` slot takes its case with its
  sign in every character;
- whole waves: in ``sorted`` the guard, the switch and (nav_lag = 1) the unwritten message are each set in every lane of some wave
  in one launch, the guard and the unwritten message also in the K = 1 launch;
- mixed waves: some wave of ``mixed``, in one launch, holds an unwritten message (nav_lag = 1) next to lanes of each Sheppard case;
  some wave holds lanes with and without the guard;
- the either-way rule (``_actuators.kept``, with BSK_T_SBR under the state bound and the guidance bits equal in the +-1e-13 runs)
  leaves out at most 2 % of the characters outside ``tie`` and keeps 12 of 16 (48 of 64) in every slot.

The per-slot branch table, the share left out and the 50-digit worst errors are printed."""
import numpy as np
import pytest

import _actuators as A
import _guidance as G
from oracle import oracle


@pytest.fixture(scope="module")
def masklib(tmp_path_factory):
    return oracle.build_branch_mask(tmp_path_factory.mktemp("oracle_branch_mask"))


def _configs():
    seen, out = set(), []
    for form, (grav, n_rw, level, diag, _, _, _, nav, _) in G.FORMS.items():
        key = (grav, n_rw, "bare" if level == "ldss" else level, diag, nav)
        if key not in seen:
            seen.add(key)
            out.append(form)
    return out


def test_forms_cover_the_levels_and_wheel_sets():
    """bare, power and full casts with 3 and 4 wheels, one bare cast without wheels, both nav_lag settings where a form allows"""
    have = {(("bare" if r[2] == "ldss" else "full" if r[2] == "fullg" else r[2]), r[1]) for r in G.FORMS.values()}
    assert {(lvl, w) for lvl in ("bare", "power", "full") for w in (3, 4)} | {("bare", 0)} <= have
    assert set(G.FORMS) == set(A.WHEEL_FORMS) | set(A.DESAT_FORMS) | {"bare-no-wheels"}
    assert sum(G.KS) < 200 and len(G.KS) == 12 and max(G.KS) >= 60 and G.KS[0] >= 16 and G.KS[G.RESET_BEFORE] == 1 and 3 in G.KS


@pytest.mark.parametrize("form", _configs())
def test_cast_takes_every_branch_where_the_layouts_need_it(form, masklib, capsys):
    cfg, cast, _ = G.cast_for(form)
    with capsys.disabled():
        G.prove(cast, masklib)
    lay = cast.layouts()
    assert sorted(lay["sorted"]) == list(range(cast.M)) and sorted(lay["mixed"]) == list(range(cast.M))
    assert 192 <= cast.M <= 512 and lay["embedded"].size == A.N_EMBEDDED and (lay["embedded"][:A.OFFSET] < 0).all()
    for w, s in zip(A.waves(lay["sorted"])[:3], ("guard", "cross", "znav")):
        assert (cast.slot[w] == s).all()
    assert np.abs(np.linalg.norm(list(cfg.sigma_R0N)) - 0.9) < 0.01


def test_either_way_rule_sees_a_character_on_the_guard_edge(masklib):
    """A ``near`` character moved ONTO |den| = 0.1 to the last bit that bisection reaches is left out, and only that one: one scaled
    run takes the guard where the other does not."""
    cfg, cast, _ = G.cast_for("bare-diag/nav1")
    saved = cast.state
    try:
        cast.state = saved.copy()
        c = int(cast.where("near")[1])                                  # (odd: action 1, the reference is sigma_R0N)
        sR = np.array(list(cfg.sigma_R0N))
        far, close = cast.state[6:9, c].copy(), cast.state[6:9, int(cast.where("guard")[1])].copy()
        assert abs(G.submrp_raw(far, sR)[0]) > 0.1 > abs(G.submrp_raw(close, sR)[0])
        lo, hi = 0.0, 1.0
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if abs(G.submrp_raw(far + mid * (close - far), sR)[0]) >= 0.1 else (lo, mid)
        base = A.kept(cast, sbr=True, lib=masklib, bits=G.ALL)
        cast.state[6:9, c] = far + hi * (close - far)
        ok = A.kept(cast, sbr=True, lib=masklib, bits=G.ALL)
        assert not ok[c] and base[c] and np.array_equal(np.delete(ok, c), np.delete(base, c)), (ok[c], base[c], int((~ok).sum()), int((~base).sum()))
    finally:
        cast.state = saved


def test_the_flip_changes_no_tracking_error():
    """Why a kernel WITHOUT the b0 < 0 flip passes tests/test_gpu_guidance.py (its mutation table): the flip only chooses the MRP set
    of sigma_RN, sigma_RN feeds nothing but ``submrp``, and ``submrp``'s result - mapped to the inner set - does not depend on the set
    of its second argument.  Without the flip b0 > -0.71 in cases 1 .. 3, so 1 + b0 > 0.29 amplifies nothing.  On every character of
    the flip slots: ``submrp`` against sigma_RN and against its shadow agree to 1e-13."""
    cfg, cast, _ = G.cast_for("bare-diag/nav1")
    worst, n = 0.0, 0
    for s in ("case1-", "case2-", "case3-"):
        for c in cast.where(s):
            col = cast.state[:, c]
            sR = G.sigma_ref(cfg, col, 0)
            a, b = oracle.submrp(col[6:9], sR), oracle.submrp(col[6:9], -sR / (sR @ sR))
            if abs(a @ a - 1.0) > 1e-9:
                worst, n = max(worst, float(np.abs(a - b).max())), n + 1
    assert n >= 40 and worst < 1e-13, (n, worst)


# ---------------------------------------------------------------------------------------------------------------- 50 digits
def _attitude_error(q, want, G50):
    """largest DCM entry difference between an fp64 MRP and a 50-digit one"""
    import mpmath as mp
    a, b = G50.mrp2c([mp.mpf(float(v)) for v in q]), G50.mrp2c(list(want))
    return float(max(abs(a[i][j] - b[i][j]) for i in range(3) for j in range(3)))


def test_oracle_c2mrp_and_submrp_against_50_digits(capsys):
    """Every input the oracle's ``c2mrp`` and ``submrp`` see for the casts' states as constructed (the initial and the spare states
    under the action of their launch; the Hill DCM built operation by operation as ``guidance`` builds it), the ``tie`` frames
    included, through the mpmath functions of tests/golden/make_golden.py.  Bound 1e-13 (tests/test_oracle_kat.py), for ``submrp``
    outside the guard divided by min(1, |den|).  Where the 50-digit value sits within 1e-12 of a branch edge (two b2 tied, b0 = 0,
    |den| = 0.1, |q|^2 = 1) the attitudes (DCMs) are compared instead of the MRP components."""
    import os
    import sys

    import mpmath as mp
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as G50
    M = mp.mpf
    worst = {"c2mrp": 0.0, "c2mrp at an edge (DCM)": 0.0, "submrp": 0.0, "submrp guarded": 0.0, "submrp at an edge (DCM)": 0.0}
    count = dict.fromkeys(worst, 0)
    for form in ("bare-diag/nav1", "power-pair/nav0", "bare-no-wheels"):
        cfg, cast, _ = G.cast_for(form)
        for states, call in ((cast.state, 0), (cast.spare, G.RESET_BEFORE)):
            for c in range(cast.M):
                col, action = states[:, c], int(cast.actions[call, c])
                if action == 0:
                    dcm = G.hill_dcm(col[0:3], col[3:6])
                    got = oracle.c2mrp(dcm)
                    C = [[M(float(dcm[3 * i + j])) for j in range(3)] for i in range(3)]
                    want = G50.c2mrp(C)
                    tr = C[0][0] + C[1][1] + C[2][2]
                    b2 = [(1 + tr) / 4] + [(1 + 2 * C[i][i] - tr) / 4 for i in range(3)]
                    case = max(range(4), key=lambda i: b2[i])
                    num = [M(1), C[1][2] - C[2][1], C[2][0] - C[0][2], C[0][1] - C[1][0]][case]          # b0's numerator in case 1 .. 3
                    edge = sorted(b2)[3] - sorted(b2)[2] < M("1e-12") or abs(num) < M("1e-12")
                    key = "c2mrp at an edge (DCM)" if edge else "c2mrp"
                    err = _attitude_error(got, want, G50) if edge else float(max(abs(M(float(g)) - w) for g, w in zip(got, want)))
                    worst[key], count[key] = max(worst[key], err), count[key] + 1
                    assert err < 1e-13, (form, cast.slot[c], c, key, err)
                    sR = got
                else:
                    sR = np.array(list(cfg.sigma_R0N))
                q1, q2 = [M(float(v)) for v in col[6:9]], [M(float(v)) for v in sR]
                got, want = oracle.submrp(col[6:9], sR), G50.submrp(q1, q2)
                d1, d2 = G50.dot(q1, q1), G50.dot(q2, q2)
                den = 1 + d1 * d2 + 2 * G50.dot(q1, q2)
                guarded = abs(den) < M("0.1")
                edge = abs(abs(den) - M("0.1")) < M("1e-12") or abs(G50.dot(want, want) - 1) < M("1e-12")
                key = "submrp at an edge (DCM)" if edge else "submrp guarded" if guarded else "submrp"
                err = _attitude_error(got, want, G50) if edge else float(max(abs(M(float(g)) - w) for g, w in zip(got, want)))
                bound = 1e-13 if guarded or edge else 1e-13 / min(1.0, float(abs(den)))
                worst[key], count[key] = max(worst[key], err * (1e-13 / bound)), count[key] + 1
                assert err < bound, (form, cast.slot[c], c, key, err, bound, float(den))
    with capsys.disabled():
        print("\n[guidance] the oracle against 50 digits, worst error (in units that make the bound 1e-13): "
              + ", ".join("%s %.2e over %d" % (k, worst[k], count[k]) for k in worst))
    assert count["c2mrp"] > 500 and count["submrp guarded"] > 100 and count["c2mrp at an edge (DCM)"] >= 24
