"""A cast of spacecraft that takes every data-dependent branch of the attitude guidance chain - hillPoint | inertial3D ->
attTrackingError - and of the shadow-set switch, with the layouts it is run in (tests/test_guidance_host.py,
tests/test_gpu_guidance.py).  CPU only: nothing here runs a kernel.  The other half of the FSW chain has tests/_actuators.py; this
module reuses its machinery (``Cast``'s layouts and batches, ``kept``, ``check_cap``, ``waves``, the kernel forms, ``cast_for``,
``names_for``).

The branches (csrc/bsk_device.hpp: ``hill_point<ZNAV>``, ``c2mrp``, ``submrp``, ``guidance``; oracle/bsk_oracle.c: ORC_B_GUID_* ...):
the reference choice (Hill frame, sigma_R0N, the zero reference of a navigation message nobody has written), the four Sheppard cases
of ``c2mrp`` and the b0 < 0 flip, the near-singular guard |den| < 0.1 and the inner-set map of ``submrp``, the shadow-set switch after
an RK4 step.

CAST  slots of 16 characters (three of them 64: a whole wave of ``sorted``; ``tie`` 24), every value finite.  "Constructed" slots
start with step counter 1 and tick counter 10 - nav_lag, so that the first sub-step of the first launch runs the FSW tick on the state as
constructed (without wheels there is no FSW tick: the observation's guidance sees the state after the launch).

  guard*   |den| of ``submrp`` log-uniform over [1.2e-3, 0.085].  With wheels: sigma = -s'/|s'|^2, s' = sigma_R + a small offset - the body
           within a few degrees of its reference, on the other MRP set (|den| = |s' - sigma_R|^2 / |s'|^2).  Even characters under
           action 0 on the near-pi Hill frames below (|sigma_R| = 0.7 .. 0.97), odd ones under action 1 (|sigma_R0N| = 0.9 in the
           cast's config).  Without wheels: the state must still be there after the launch, so sigma = -s sigma_R + a small normal
           part with |sigma| < 1 (|den| >= (1 - |sigma| |sigma_R|)^2: the band starts at 1.2e-2), omega = 0, L_ext = 0.
           With wheels every third and fourth character is CONVERGED on the other set instead: the offset 3e-8 .. 3e-5 of |sigma_R|,
           |den| = 1e-15 .. 1e-9 (fp64 no longer resolves it; it may round to 0).  Only there does the guard matter numerically: the
           unguarded formula is the same attitude with a relative error of 1e-16 / den in its length, invisible at the bounds of the
           GPU test down to |den| = 1e-10 (the kernel that never took the guard passed the band above)
  cross*   tests/_crowd.py's construction: mid-episode, sigma = (1 - 0.05 dt U(22, 38)) s^, omega = 0.1 s^: |sigma| reaches 1 inside the second
           launch (K = 40); after the masked reset inside the K = 1 launches (distance U(0.25, 0.75) and U(1.25, 1.75) ticks)
  znav*    fresh at tick 0, action 0: under nav_lag = 1 the t = 0 tick reads the message nobody has written
  case0    the Hill frame a rotation by 0 .. 85 degrees from the inertial frame
  case1+ case1- case2+ case2- case3+ case3-
           the Hill frame a rotation by pi - delta, delta = U(0.05, 0.6), about +-x, +-y, +-z tilted by up to 0.3 towards the other axes
           (a pure axis rotation leaves the off-axis numerators of its Sheppard case at zero).  Of the chosen DCM C: r = a C[0],
           v = v_t C[1] + v_r C[0], a = 6.8 .. 7.2e6 m, v_t within 1 % of circular, v_r = +-(100 .. 300) m/s (ddfdt2 != 0).  "-": b0 < 0, the flip
  near     the guard's construction with |den| in [0.12, 0.3]: just outside it, the worst conditioning the unguarded formula is allowed
  inner    a relative rotation beyond 180 degrees: |sigma_BR|^2 = 1.2 .. 4 before the inner-set map, |den| > 0.15; even: action 0, odd: 1
  mid      sampled states stepped 1 .. 16 ticks: every FSW phase
  track    600 .. 615 ticks under action 0: small sigma_BR on a moving reference
  tie      the 24 signed-permutation rotation matrices as Hill frames: exact ties between the b2 and exact b0 = 0 - edge characters by
           construction, exempt from the cap; across layouts they must still give the same bits
  (*: 64 characters; the first 16 of every slot are the ``base`` cast that ``embedded`` holds.)

SCHEDULE  12 launches of KS sub-steps, 181 ticks.  The first has K = 16: the pair and three-wave forms run the FSW tick on the
constructed states.  The masked host reset comes before the sixth launch, the first of K = 1 (the halves form): every character of
the constructed slots restarts from a SECOND constructed state of its slot with the same counters (``znav``: 0), so that launch runs
the FSW tick on it; ``case0``, ``mid`` and ``track`` run on.  Actions change per character across launches (0 -> 1 -> 2 -> 0: the
reference jumps); they are the same in the first and the sixth launch.

LAYOUTS  ``sorted``, ``mixed``, ``embedded`` (n = 333) as in tests/_actuators.py."""
import itertools

import numpy as np

import _actuators as A
from basilisk_env_amd import _lib
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from oracle import oracle

PER, WAVE = A.PER, A.WAVE
KS = (16, 40, 3, 7, 60, 1, 1, 5, 10, 1, 25, 12)
RESET_BEFORE = 5
assert set(KS) == set(A.KS)                                                 # (``A.names_for`` names the kernel of every K of A.KS)
SLOTS = ("guard", "cross", "znav", "case0", "case1+", "case1-", "case2+", "case2-", "case3+", "case3-", "near", "inner", "mid", "track", "tie")
COUNT = {"guard": WAVE, "cross": WAVE, "znav": WAVE, "tie": 24}
RUN_ON = ("case0", "mid", "track")                                          # not reset
EXEMPT = ("tie",)
SIGMA_R0N = (0.54, -0.60, 0.39)                                             # norm 0.896

# oracle/bsk_oracle.c: ORC_B_GUID_ZNAV ... (bits 19 .. 29) - a tuple of their own: ``A.BITS`` stays the actuator chain's
BITS = ("guid_znav", "guid_hill", "guid_inertial", "c2mrp_0", "c2mrp_1", "c2mrp_2", "c2mrp_3", "c2mrp_flip", "submrp_guard", "submrp_inner", "mrp_switch")
BIT = {name: np.uint32(1 << (19 + i)) for i, name in enumerate(BITS)}
ALL = np.uint32(sum(int(b) for b in BIT.values()))
# the slot that exists for each bit
HOME = {"guid_znav": ("znav",), "guid_hill": ("case0",), "guid_inertial": ("guard",), "c2mrp_0": ("case0",), "c2mrp_1": ("case1+", "case1-"),
        "c2mrp_2": ("case2+", "case2-"), "c2mrp_3": ("case3+", "case3-"), "c2mrp_flip": ("case1-", "case2-", "case3-"),
        "submrp_guard": ("guard",), "submrp_inner": ("inner",), "mrp_switch": ("cross",)}
ACT0 = np.array([0, 0, 1, 2, 0, 0, 0, 1, 2, 0, 1, 0])                        # per launch; the same at 0 and at RESET_BEFORE
ACT1 = np.array([1, 1, 2, 0, 0, 1, 1, 2, 0, 1, 0, 0])


def guidance_config(cfg):
    """The cast's edit of a form's config (in place): a sigma_R0N of norm 0.9 (the default has norm 1, on the edge of both sets)"""
    for k in range(3):
        cfg.sigma_R0N[k] = SIGMA_R0N[k]
    return cfg


# ---------------------------------------------------------------------------------------------------------------- formulae
def hill_dcm(r, v):
    """The Hill frame's DCM as the oracle's ``guidance`` builds it, operation by operation (fp64, no fused arithmetic) -> (9,)"""
    cr = lambda a, b: np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])      # noqa: E731
    nm = lambda a: np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])                                                    # noqa: E731
    h = cr(r, v)
    i_r, i_h = (1.0 / nm(r)) * r, (1.0 / nm(h)) * h
    return np.concatenate([i_r, cr(i_h, i_r), i_h])


def sigma_ref(cfg, col, action):
    """sigma_RN of a state column under an action, to the oracle's bits"""
    return oracle.c2mrp(hill_dcm(col[0:3], col[3:6])) if action == 0 else np.array(list(cfg.sigma_R0N))


def submrp_raw(q1, q2):
    """``submrp`` without its guard and its map -> den, |q|^2"""
    d1, d2 = q1 @ q1, q2 @ q2
    den = 1.0 + d1 * d2 + 2.0 * (q1 @ q2)
    with np.errstate(all="ignore"):
        q = ((1.0 - d2) * q1 - (1.0 - d1) * q2 + 2.0 * np.cross(q1, q2)) / den
    return den, q @ q


def tie_frames():
    """the 24 rotation matrices whose entries are 0, +-1"""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1.0, -1.0), repeat=3):
            C = np.zeros((3, 3))
            for i in range(3):
                C[i, perm[i]] = signs[i]
            if np.linalg.det(C) > 0:
                out.append(C)
    assert len(out) == 24
    return out


class Cast(A.Cast):
    """``A.Cast`` with the guidance slots, a schedule of its own and counters for the spare states (spare_steps, spare_ticks)"""

    def __init__(self, cfg, kind="guidance", sh=(None, None)):
        from basilisk_env_amd._lib import FLAG_DRAG, FLAG_POWER
        self.cfg, self.sh, self.n_rw = cfg, sh, cfg.n_rw
        self.kind = "full" if cfg.flags & FLAG_DRAG else "power" if cfg.flags & FLAG_POWER else "bare"       # the level
        self.navlag = int(bool(cfg.nav_lag) and cfg.n_rw > 0)
        self.slots = SLOTS
        self.count = {s: COUNT.get(s, PER) for s in SLOTS}
        self.slot = np.concatenate([np.repeat(s, self.count[s]) for s in SLOTS])
        self.M = self.slot.size
        self.base = np.concatenate([np.arange(self.count[s]) < PER for s in SLOTS])
        self._build()

    # ------------------------------------------------------------------------------------------------------------ construction
    def _orbit(self, col, C, rng):
        """r, v of a column so that the Hill frame's DCM is C"""
        a = rng.uniform(6.8e6, 7.2e6)
        v_t, v_r = np.sqrt(self.cfg.mu / a) * rng.uniform(0.99, 1.01), rng.choice((-1.0, 1.0)) * rng.uniform(100.0, 300.0)
        col[0:3], col[3:6] = a * C[0], v_t * C[1] + v_r * C[0]

    def _near_pi(self, rng, axis, sign, delta=(0.05, 0.6)):
        e = rng.uniform(-0.3, 0.3, 3)
        e[axis] = 1.0
        e *= sign / np.linalg.norm(e)
        return oracle.mrp2c(np.tan(0.25 * (np.pi - rng.uniform(*delta))) * e)

    def _opposite(self, col, action, band, rng):
        """sigma of a column near its reference's attitude but on the other MRP set, |den| log-uniform over ``band``"""
        sR = sigma_ref(self.cfg, col, action)
        for _ in range(10000):
            want = np.exp(rng.uniform(np.log(band[0]), np.log(band[1])))
            d = rng.normal(size=3)
            if self.n_rw:
                s1 = sR + d * (np.sqrt(want) * np.linalg.norm(sR) / np.linalg.norm(d))
                s = -s1 / (s1 @ s1)
            else:
                d -= (d @ sR) / (sR @ sR) * sR
                s = -rng.uniform(0.6, 1.0 / (sR @ sR)) * sR + d * (rng.uniform(0.0, 0.1) / np.linalg.norm(d))
                if s @ s > 0.98:
                    continue
            den, _ = submrp_raw(s, sR)
            if (band[0] < 1e-6 or band[0] * 1.05 < abs(den)) and abs(den) < band[1] / 1.05:       # (below 1e-6 fp64 does not resolve den)
                col[6:9] = s
                return
        raise AssertionError("no state in the band")

    def _slot(self, name, k, take, rng, spare=False):
        """-> state (n_fields, k), steps, ticks, actions (12, k) of one slot (``spare``: its second draw, for the masked reset)"""
        cfg, n_rw, sh = self.cfg, self.n_rw, self.sh
        tail = _lib.NF_BASE + n_rw
        i = np.arange(k)
        st = take(k)
        s, t = np.ones(k, np.int32), np.full(k, 10 - self.navlag, np.int32)
        act = np.repeat(ACT0[:, None], k, axis=1)
        odd = i % 2 == 1
        if name in ("guard", "near", "inner"):
            act[:, odd] = ACT1[:, None]
        if name == "znav":
            s, t = np.zeros(k, np.int32), np.zeros(k, np.int32)
        elif name == "case0":
            for c in range(k):
                e = rng.normal(size=3)
                self._orbit(st[:, c], oracle.mrp2c(np.tan(0.25 * np.radians(rng.uniform(0.0, 85.0))) * e / np.linalg.norm(e)), rng)
        elif name.startswith("case"):
            for c in range(k):
                self._orbit(st[:, c], self._near_pi(rng, int(name[4]) - 1, 1.0 if name[5] == "+" else -1.0), rng)
        elif name == "tie":
            for c, C in enumerate(tie_frames()):
                self._orbit(st[:, c], C, rng)
        elif name in ("guard", "near"):
            band = (1.2e-3 if n_rw else 1.2e-2, 0.085) if name == "guard" else (0.12, 0.3)
            for c in range(k):
                if not odd[c]:
                    self._orbit(st[:, c], self._near_pi(rng, int(rng.integers(3)), rng.choice((-1.0, 1.0)), (0.05, 0.6) if n_rw else (0.05, 0.25)), rng)
                if not n_rw:
                    st[9:12, c], st[tail + _lib.T_LEXT:tail + _lib.T_LEXT + 3, c] = 0.0, 0.0
                converged = name == "guard" and n_rw and c % 4 >= 2
                self._opposite(st[:, c], int(act[0, c]), (1e-15, 1e-9) if converged else band, rng)
        elif name == "inner":
            for c in range(k):
                sR = sigma_ref(cfg, st[:, c], int(act[0, c]))
                for _ in range(10000):
                    q = rng.normal(size=3)
                    q *= rng.uniform(1.1, 2.0) / np.linalg.norm(q)
                    body = ((1.0 - sR @ sR) * q + (1.0 - q @ q) * sR - 2.0 * np.cross(q, sR)) / (1.0 + (sR @ sR) * (q @ q) - 2.0 * (sR @ q))
                    if body @ body > 1.0:
                        body = -body / (body @ body)
                    den, m = submrp_raw(body, sR)
                    if abs(den) > 0.15 and 1.2 < m < 4.0:
                        break
                else:
                    raise AssertionError("no inner state")
                st[6:9, c] = body
        elif name == "cross":
            if not spare:
                st, s, t = A._prerun(cfg, sh, st, 5 + i % PER, 1)
            shat = rng.normal(size=(3, k))
            shat /= np.linalg.norm(shat, axis=0)
            ticks_away = np.where(odd, rng.uniform(1.25, 1.75, k), rng.uniform(0.25, 0.75, k)) if spare else rng.uniform(22.0, 38.0, k)
            st[6:9], st[9:12] = shat * (1.0 - 0.05 * cfg.dt * ticks_away), 0.1 * shat
            act = rng.integers(0, 3, (len(KS), k))
        elif name == "mid":
            st, s, t = A._prerun(cfg, sh, st, 1 + i % PER, 1)
            act = ACT0[(np.arange(len(KS))[:, None] + i[None, :]) % len(KS)]
        elif name == "track":
            st, s, t = A._prerun(cfg, sh, st, 600 + i, 0, first=0)
        return st, np.asarray(s, np.int32), np.asarray(t, np.int32), act

    def _build(self):
        cfg, n_rw = self.cfg, self.n_rw
        rng = np.random.default_rng([29, n_rw, ("bare", "power", "full").index(self.kind), self.navlag, int(cfg.gravity_model)])
        pool = sample_ic_batch(1500, n_rw, seed=2900 + n_rw)
        nxt = iter(range(pool.shape[1]))
        take = lambda k: np.ascontiguousarray(pool[:, [next(nxt) for _ in range(k)]])       # noqa: E731
        made = [self._slot(s, self.count[s], take, rng) for s in SLOTS]
        self.state = np.ascontiguousarray(np.concatenate([m[0] for m in made], axis=1))
        self.steps, self.ticks = np.concatenate([m[1] for m in made]), np.concatenate([m[2] for m in made])
        self.actions = np.concatenate([m[3] for m in made], axis=1).astype(np.int32)
        self.reset_mask = ~np.isin(self.slot, RUN_ON)
        again = [self._slot(s, self.count[s], take, rng, spare=True) if s not in RUN_ON else (take(self.count[s]),) + made[j][1:3]
                 for j, s in enumerate(SLOTS)]
        self.spare = np.ascontiguousarray(np.concatenate([m[0] for m in again], axis=1))
        self.spare_steps, self.spare_ticks = np.concatenate([m[1] for m in again]), np.concatenate([m[2] for m in again])
        nf = A.N_EMBEDDED - int(self.base.sum())
        self.filler = A._prerun(cfg, self.sh, take(nf), 5 + np.arange(nf) % 7, 1)
        assert np.isfinite(self.state).all() and np.isfinite(self.spare).all() and np.isfinite(self.filler[0]).all()

    # ------------------------------------------------------------------------------------------------------------ the reset
    def batch_reset_counters(self, index, steps, ticks):
        """The counters of a handle after the masked reset (which zeroes them): the reset characters' own -> steps, ticks"""
        m = self.batch_reset(index)[1].astype(bool)
        c = np.maximum(index, 0)
        return np.where(m, self.spare_steps[c], steps).astype(np.int32), np.where(m, self.spare_ticks[c], ticks).astype(np.int32)

    # ------------------------------------------------------------------------------------------------------------ oracle
    def run_oracle(self, lib=None, scale=None):
        """``A.Cast.run_oracle`` under this module's schedule; ``scale`` moves every slot (there is no ``rest``)"""
        st, steps, ticks, spare = self.state.copy(), self.steps.copy(), self.ticks.copy(), self.spare.copy()
        if scale is not None:
            nd = 12 + self.n_rw
            st[:nd] *= scale
            spare[:nd] *= scale
        out = []
        for call, k in enumerate(KS):
            if call == RESET_BEFORE:
                m = self.reset_mask
                st[:, m], steps[m], ticks[m] = spare[:, m], self.spare_steps[m], self.spare_ticks[m]
            t0 = ticks.copy()
            o = oracle.step(self.cfg, st, steps, ticks, self.actions[call], k, cbar=self.sh[0], sbar=self.sh[1], lib=lib)
            rec = {"state": st.copy(), "obs": o[0], "reward": o[1], "reason": o[3], "steps": steps.copy(), "ticks": ticks.copy(), "ticks0": t0}
            if lib is not None:
                rec["mask"] = oracle.branch_masks(lib, self.M)
            out.append(rec)
        return out


# ---------------------------------------------------------------------------------------------------------------- proofs
def prove(cast, masklib, verbose=True):
    """The conditions of tests/test_guidance_host.py from the branch masks -> runs (with masks), kept (M,), the printed lines"""
    cfg, nav = cast.cfg, cast.navlag
    runs, plain = cast.run_oracle(lib=masklib), cast.run_oracle()
    for a, b in zip(runs, plain):                                      # the instrumented build computes the same bits
        for key in b:
            same = np.array_equal(a[key].view(np.uint64), b[key].view(np.uint64)) if b[key].dtype == np.float64 else np.array_equal(a[key], b[key])
            assert same, key
    report = {}
    ok = A.kept(cast, runs, report, sbr=True, lib=masklib, bits=ALL)
    mask = np.array([r["mask"] for r in runs])                          # (launches, M)
    has = {name: (mask & BIT[name]) != 0 for name in BITS}
    carried = [b for b in BITS if b != "guid_znav" or nav]
    lines = ["%-14s %s" % ("bit", " ".join("%6s" % s[:6] for s in SLOTS))]
    for name in BITS:
        lines.append("%-14s %s" % (name, " ".join("%6d" % int(has[name].any(axis=0)[cast.where(s)].sum()) for s in SLOTS)))
        for home in HOME[name] if name in carried else ():
            w = cast.where(home)
            for call in (0, RESET_BEFORE) if cast.n_rw and home not in RUN_ON + ("cross",) else (None,):
                took = has[name].any(axis=0) if call is None else has[name][call]
                assert (took[w] & ok[w]).sum() >= 8, (cast.kind, cast.n_rw, nav, name, home, call, int((took[w] & ok[w]).sum()))
    if not nav:
        assert not has["guid_znav"].any()
    # the intended case with the intended sign, on the state as constructed (with wheels: the first launch's FSW tick)
    if nav:                                                             # (nav_lag = 0: the observation's guidance adds its own)
        for axis in (1, 2, 3):
            for sign in "+-":
                w = cast.where("case%d%s" % (axis, sign))
                m0 = mask[0, w]
                assert ((m0 & BIT["c2mrp_%d" % axis]) != 0).all() and (((m0 & BIT["c2mrp_flip"]) != 0) == (sign == "-")).all(), (axis, sign)
                assert not (m0 & (BIT["c2mrp_0"] | sum(BIT["c2mrp_%d" % o] for o in (1, 2, 3) if o != axis))).any(), (axis, sign)
        assert (mask[0, cast.where("case0")] & (BIT["c2mrp_1"] | BIT["c2mrp_2"] | BIT["c2mrp_3"])).max() == 0
        assert not has["submrp_guard"][0, cast.where("near")].any()
    lay = cast.layouts()
    srt, mixed = A.waves(lay["sorted"]), A.waves(lay["mixed"])

    def every_lane(pred, what, calls=None):                             # in one launch, every lane of some whole wave of sorted
        calls = range(len(KS)) if calls is None else calls
        assert any(pred[c, w].all() for c in calls for w in srt if w.size == WAVE), (cast.kind, cast.n_rw, nav, what, "in every lane of no wave of sorted")

    every_lane(has["submrp_guard"], "guard")
    every_lane(has["mrp_switch"], "shadow-set switch")
    if nav:
        every_lane(has["guid_znav"], "unwritten message")
        # the K = 1 launch after the masked reset (the halves form's): whole waves of the guard and of the unwritten message in it,
        # the switch inside it and inside the next
        assert KS[RESET_BEFORE] == 1 and KS[RESET_BEFORE + 1] == 1
        every_lane(has["submrp_guard"], "guard, K = 1", (RESET_BEFORE,))
        every_lane(has["guid_znav"], "unwritten message, K = 1", (RESET_BEFORE,))
        cr = cast.where("cross")
        for c in (RESET_BEFORE, RESET_BEFORE + 1):
            assert (has["mrp_switch"][c, cr] & ok[cr]).sum() >= 8, (c, int((has["mrp_switch"][c, cr] & ok[cr]).sum()))
    cases = [has["c2mrp_%d" % i] for i in range(4)]
    assert any(all(p[c, w].any() for p in cases + ([has["guid_znav"]] if nav else [])) for c in range(len(KS)) for w in mixed), "no wave of mixed with every case"
    assert any(has["submrp_guard"][c, w].any() and not has["submrp_guard"][c, w].all() for c in range(len(KS)) for w in mixed), "no wave of mixed with and without the guard"
    share = A.check_cap(cast, ok, EXEMPT)
    tie = cast.where("tie")
    lines.append("either-way rule: %.2f %% of the %d characters outside tie left out (%s); tie keeps %d of %d; under the 1e-13 scaling the oracle "
                 "moves by %.2f of a GPU bound, its sign-independent part by %.4f"
                 % (100.0 * share, cast.M - tie.size, {s: int((~ok[cast.where(s)]).sum()) for s in SLOTS if s not in EXEMPT and (~ok[cast.where(s)]).any()},
                    int(ok[tie].sum()), tie.size, report["plain"], report["symmetric"]))
    if verbose:
        print("\n[guidance cast, %s, %d wheels, nav_lag %d] characters that take each branch, per slot\n" % (cast.kind, cast.n_rw, cfg.nav_lag) + "\n".join(lines))
    return runs, ok, lines


# ---------------------------------------------------------------------------------------------------------------- the forms
def _forms():
    from basilisk_env_amd._lib import GRAV_PM_J2
    out = dict(A.WHEEL_FORMS)
    out.update(A.DESAT_FORMS)
    out["bare-no-wheels"] = (GRAV_PM_J2, 0, "bare", True, "0", "0", None, 1, "step")
    return out


FORMS = _forms()


def cast_for(form):
    """(cfg, Cast, row) of one entry of FORMS (``A.cast_for`` with this module's cast and config edit)"""
    return A.cast_for("guidance", form, forms=FORMS, edit=guidance_config, make=Cast)
