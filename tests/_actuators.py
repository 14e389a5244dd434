"""Two casts of spacecraft that take every data-dependent branch of the wheel and thruster command chain, and the layouts they are
run in (tests/test_actuators_host.py, tests/test_gpu_actuators.py).  CPU only: nothing here runs a kernel.  In the style of
tests/_crowd.py, whose cast covers the physics regimes; this one covers the actuator chain: the u_max clamp and the u_min dead-band of
``control``, Coulomb friction at a wheel's zero crossing and at rest, every branch of the desaturation tick, and the wave-uniform
burst decisions (``ev.thr_on``, ``burst_any``, ``uni_any`` of csrc/bsk_kernels.hip).

CAST  slots of 16 characters (four of them 64: a whole wave of ``sorted``), every value finite.

  wheel cast (bare and power levels, 3 or 4 wheels; nav_lag 0 or 1)
    rest*    every wheel exactly 0, sigma = sigma_R0N, omega = 0, L_ext = 0, action 1.  nav_lag = 0: the command is exactly zero and the
             wheels stay exactly at rest; nav_lag = 1: the t = 0 tick reads empty messages and they leave rest when its command arrives
    cross*   sampled attitude, wheel speeds U(-0.05, 0.05) rad/s, actions 0 / 1: kept are candidates of which a wheel changes sign
    dead     mid-episode (ticks 1 .. 16), sigma = sigma_R0N + 1e-7 U(-1, 1), omega = 0, wheels 0 (a turning wheel's friction torque
             alone moves the hub past the dead-band within a second), L_ext = 0, action 1: non-zero commands below u_min
    sat      sampled tumble, wheels x 2.5, omega x 40: clamped commands
    pass     600 ticks under action 1: close to its target, small commands above the dead-band
    mid      sampled, stepped 1 .. 16 ticks: every FSW phase

  desat cast (power, Sun third body, drag, desaturation; thr_min_fire_time 0.3, thr_min_on_time 0.6, thr_max_counter 1, fsw_every 10,
  dt 0.1: the dropped, stretched and partial bands of a pulse are each wide, a stretched pulse has the burst limit 12)
    dump*    mid-episode, wheels x 2.5, action 2 throughout (a new request at the first FSW tick of every launch)
    stagger* the same at tick counters 1 .. 16: bursts start and end in different ticks per lane
    below    wheels x 0.05: momentum under hs_min, the request dumps nothing, yet a burst of zeros is latched
    t0       fresh at tick 0 in mode 2, wheels x 2.5: under nav_lag = 1 the request reads messages nobody wrote
    leave    action 2, then 1: the running burst finishes and no new one starts
    reenter  actions 2, 1, 2, ...: the new request resets a running schedule
    idle     never action 2
    reset    action 2 from ticks 8 / 9: the masked host reset falls in the middle of a burst
    rest*, cross*, dead   as above
  (*: 64 characters; the first 16 of every slot are the ``base`` cast that every layout holds.)

SCHEDULE  12 launches of KS sub-steps, 181 ticks; the third (K = 3) holds no FSW tick for a character that started at tick 0; K >= 16
selects the pair / three-wave forms where they are built; the masked host reset (every fifth character and the whole ``reset`` slot,
from the cast's spare states) comes after the third launch.

LAYOUTS  ``sorted`` (whole waves of one slot: the 64-character slots first), ``mixed`` (every wave a proportional share of every
slot), ``embedded`` (n = 333, the base cast at offset 37 in benign filler)."""
import numpy as np

from basilisk_env_amd import _lib
from basilisk_env_amd._lib import FLAG_DESAT
from basilisk_env_amd.simulators.initial_conditions.batch import sample_ic_batch
from oracle import oracle

PER, WAVE = 16, 64
N_EMBEDDED, OFFSET = 333, 37
KS = (10, 40, 3, 7, 60, 1, 1, 5, 16, 1, 25, 12)
RESET_BEFORE = 3
SLOTS = {"wheel": ("rest", "cross", "dead", "sat", "pass", "mid"),
         "desat": ("dump", "stagger", "rest", "cross", "below", "t0", "leave", "reenter", "idle", "reset", "dead")}
WHOLE_WAVE = ("dump", "stagger", "rest", "cross")

# oracle/bsk_oracle.c: ORC_B_*
BITS = ("req_above", "req_below", "tick_fire", "tick_count", "pulse_drop_owed", "pulse_drop_zero", "pulse_full", "pulse_stretch",
        "pulse_partial", "cmd_clamp", "cmd_dead", "cmd_zero", "cmd_pass", "om_pos", "om_neg", "om_zero", "thr_stage", "thr_end", "om_cross")
BIT = {name: np.uint32(1 << i) for i, name in enumerate(BITS)}
CARRIED = {"wheel": BITS[9:16] + ("om_cross",), "desat": BITS}


def desat_config(cfg):
    """The desat cast's edits of a full-scenario config (in place)"""
    cfg.thr_min_fire_time, cfg.thr_min_on_time, cfg.thr_max_counter = 0.3, 0.6, 1
    cfg.fsw_every, cfg.dt = 10, 0.1
    return cfg


def _prerun(cfg, sh, st, js, action, first=1):
    """each column of ``st`` stepped js[i] ticks by the oracle: an env step of one tick under ``first`` (it takes the t = 0 FSW tick),
    then one of js[i] - 1 ticks under ``action`` -> state, steps (all 1: mid-episode, far from max_length), ticks"""
    out, ticks = st.copy(), np.zeros(st.shape[1], np.int32)
    js = np.asarray(js)
    for j in np.unique(js):
        w = np.flatnonzero(js == j)
        col, s, t = np.ascontiguousarray(st[:, w]), np.zeros(w.size, np.int32), np.zeros(w.size, np.int32)
        oracle.step(cfg, col, s, t, np.full(w.size, first, np.int32), 1, cbar=sh[0], sbar=sh[1])
        if j > 1:
            oracle.step(cfg, col, s, t, np.full(w.size, action, np.int32), int(j) - 1, cbar=sh[0], sbar=sh[1])
        out[:, w], ticks[w] = col, t
    return out, np.ones(st.shape[1], np.int32), ticks


class Cast(object):
    """state (n_fields, M), steps, ticks (M,): what each character starts from; spare (n_fields, M): its fresh state at the masked
    reset; actions (12, M); slot (M,) names; base (M,) bool; filler (state, steps, ticks) of benign spacecraft for ``embedded``."""

    def __init__(self, cfg, kind, sh=(None, None)):
        assert kind in SLOTS and cfg.n_rw > 0 and (kind == "wheel" or cfg.flags & FLAG_DESAT)
        self.cfg, self.kind, self.sh, self.n_rw = cfg, kind, sh, cfg.n_rw
        self.slots = SLOTS[kind]
        self.count = {s: WAVE if s in WHOLE_WAVE else PER for s in self.slots}
        self.slot = np.concatenate([np.repeat(s, self.count[s]) for s in self.slots])
        self.M = self.slot.size
        self.base = np.concatenate([np.arange(self.count[s]) < PER for s in self.slots])
        self._build()

    def where(self, name):
        return np.flatnonzero(self.slot == name)

    # ------------------------------------------------------------------------------------------------------------ construction
    def _crossers(self, cand, acts):
        """of the candidate ``cross`` states, the first 64 of which a wheel changes sign within the first two launches, under the
        character's own actions (tick by tick on the oracle) -> their columns"""
        cfg, n_rw, n = self.cfg, self.n_rw, cand.shape[1]
        st, steps, ticks = cand.copy(), np.zeros(n, np.int32), np.zeros(n, np.int32)
        sign0, crossed = np.sign(st[12:12 + n_rw]), np.zeros(n, bool)
        for call in (0, 1):
            for _ in range(KS[call]):
                oracle.step(cfg, st, steps, ticks, acts[call], 1, cbar=self.sh[0], sbar=self.sh[1])
                crossed |= (np.sign(st[12:12 + n_rw]) * sign0 < 0).any(axis=0)
        keep = np.flatnonzero(crossed)[:WAVE]
        assert keep.size == WAVE, keep.size
        return keep

    def _build(self):
        cfg, n_rw, kind, sh = self.cfg, self.n_rw, self.kind, self.sh
        tail = _lib.NF_BASE + n_rw
        rng = np.random.default_rng([23, n_rw, len(kind), int(cfg.nav_lag)])
        pool = sample_ic_batch(1200, n_rw, seed=2300 + n_rw)
        nxt = iter(range(pool.shape[1]))
        take = lambda k: np.ascontiguousarray(pool[:, [next(nxt) for _ in range(k)]])       # noqa: E731
        sig0 = np.array(list(cfg.sigma_R0N))
        L = len(KS)
        state, steps, ticks, actions = [], [], [], []
        for name in self.slots:
            k = self.count[name]
            i = np.arange(k)
            s, t = np.zeros(k, np.int32), np.zeros(k, np.int32)
            act = rng.integers(0, 3 if kind == "wheel" else 2, (L, k))
            if name == "rest":
                st = take(k)
                st[6:9], st[9:12], st[12:12 + n_rw] = sig0[:, None], 0.0, 0.0
                st[tail + _lib.T_LEXT:tail + _lib.T_LEXT + 3] = 0.0
                act[:] = 1
            elif name == "cross":
                cand = take(2 * k)
                cand[12:12 + n_rw] = rng.uniform(-0.05, 0.05, (n_rw, 2 * k))
                a2 = rng.integers(0, 2, (L, 2 * k))
                keep = self._crossers(cand, a2)
                st, act = cand[:, keep], a2[:, keep]
            elif name == "dead":
                st = take(k)
                st[6:9], st[9:12], st[12:12 + n_rw] = sig0[:, None] + 1e-7 * rng.uniform(-1.0, 1.0, (3, k)), 0.0, 0.0
                st[tail + _lib.T_LEXT:tail + _lib.T_LEXT + 3] = 0.0
                s, t = np.ones(k, np.int32), (1 + i % PER).astype(np.int32)
                act[:] = 1
            elif name == "sat":
                st = take(k)
                st[12:12 + n_rw] *= 2.5
                st[9:12] *= 40.0
            elif name == "pass":
                st, s, t = _prerun(cfg, sh, take(k), 600 + i, 1)
            elif name in ("mid", "idle"):
                st, s, t = _prerun(cfg, sh, take(k), 1 + i % PER, 1)
            elif name in ("dump", "stagger", "leave", "reenter", "below", "reset"):
                st = take(k)
                st[12:12 + n_rw] *= 0.05 if name == "below" else 2.5
                j = {"dump": 21 + (3 * i) % 20, "stagger": 1 + i % PER, "reset": 8 + i % 2}.get(name, 3 + i)
                st, s, t = _prerun(cfg, sh, st, j, 1)
                act[:] = 2
                if name == "leave":
                    act[1:] = 1
                if name == "reenter":
                    act[1::3] = 1
            elif name == "t0":
                st = take(k)
                st[12:12 + n_rw] *= 2.5
                act = rng.integers(1, 3, (L, k))
                act[0] = 2
            state.append(st)
            steps.append(s)
            ticks.append(t)
            actions.append(act)
        self.state = np.ascontiguousarray(np.concatenate(state, axis=1))
        self.steps, self.ticks = np.concatenate(steps).astype(np.int32), np.concatenate(ticks).astype(np.int32)
        self.actions = np.concatenate(actions, axis=1).astype(np.int32)
        self.reset_mask = (np.arange(self.M) % 5 == 0) | (self.slot == "reset")
        self.spare = take(self.M)
        if kind == "desat":
            self.spare[12:12 + n_rw] *= 2.5
        rest = self.where("rest")
        self.spare[:, rest] = self.state[:, rest]                          # a wheel at rest restarts at rest
        fst, fs, ft = _prerun(cfg, sh, take(N_EMBEDDED - int(self.base.sum())), 5 + np.arange(N_EMBEDDED - int(self.base.sum())) % 7, 1)
        self.filler = (fst, fs, ft)
        assert np.isfinite(self.state).all() and np.isfinite(self.spare).all() and np.isfinite(fst).all()

    # ------------------------------------------------------------------------------------------------------------ layouts
    def layouts(self):
        """-> {name: index (n,) int: the character in each env, -1 filler}"""
        first = [s for s in self.slots if self.count[s] == WAVE] + [s for s in self.slots if self.count[s] != WAVE]
        srt = np.concatenate([self.where(s) for s in first])
        frac = np.concatenate([(np.arange(self.count[s]) + 0.5) / self.count[s] for s in self.slots])
        mixed = np.lexsort((np.arange(self.M), frac))
        emb = np.full(N_EMBEDDED, -1)
        emb[OFFSET:OFFSET + int(self.base.sum())] = np.flatnonzero(self.base)
        return {"sorted": srt, "mixed": mixed, "embedded": emb}

    def batch(self, index):
        """-> (state, steps, ticks) of a handle whose env e holds character index[e] (-1: the next filler spacecraft)"""
        f = np.cumsum(index < 0) - 1
        pick = lambda c, fl: np.where(index >= 0, c[..., np.maximum(index, 0)], fl[..., np.maximum(f, 0)])      # noqa: E731
        return (np.ascontiguousarray(pick(self.state, self.filler[0])), pick(self.steps, self.filler[1]).astype(np.int32),
                pick(self.ticks, self.filler[2]).astype(np.int32))

    def batch_actions(self, index, call):
        return np.where(index >= 0, self.actions[call][np.maximum(index, 0)], 1).astype(np.int32)

    def batch_reset(self, index):
        """-> (fresh (n_fields, n), mask (n,) uint8) of the masked reset, each character from its own spare state"""
        fresh = np.ascontiguousarray(self.spare[:, np.maximum(index, 0)])
        return fresh, ((index >= 0) & self.reset_mask[np.maximum(index, 0)]).astype(np.uint8)

    # ------------------------------------------------------------------------------------------------------------ oracle
    def run_oracle(self, lib=None, scale=None):
        """The schedule on the oracle, the cast in its own order -> per launch a dict of copies: state, obs, reward, reason, steps,
        ticks, ticks0 (before the launch) and, with a branch-mask build as ``lib``, mask.  ``scale``: the dynamic rows of the
        initial and the spare states multiplied by it (the either-way rule; the ``rest`` slot exempt - zero stays zero)."""
        st, steps, ticks, spare = self.state.copy(), self.steps.copy(), self.ticks.copy(), self.spare.copy()
        if scale is not None:
            moved, nd = self.slot != "rest", 12 + self.n_rw
            for a in (st, spare):
                a[:nd, moved] *= scale
        out = []
        for call, k in enumerate(KS):
            if call == RESET_BEFORE:
                m = self.reset_mask
                st[:, m], steps[m], ticks[m] = spare[:, m], 0, 0
            t0 = ticks.copy()
            o = oracle.step(self.cfg, st, steps, ticks, self.actions[call], k, cbar=self.sh[0], sbar=self.sh[1], lib=lib)
            rec = {"state": st.copy(), "obs": o[0], "reward": o[1], "reason": o[3], "steps": steps.copy(), "ticks": ticks.copy(), "ticks0": t0}
            if lib is not None:
                rec["mask"] = oracle.branch_masks(lib, self.M)
            out.append(rec)
        return out


# ---------------------------------------------------------------------------------------------------------------- either-way rule
STATE_BOUND, REM_BOUND, CMD_BOUND = 1e-11, 1e-12, 1e-11        # tests/test_gpu_actuators.py


def column_errors(a, b, n_rw):
    """per character: the largest error of a state group relative to the group's largest magnitude in ``b`` (helpers.max_group_err,
    column by column) -> (M,)"""
    from helpers import field_groups
    worst = np.zeros(a.shape[1])
    for sl in field_groups(n_rw).values():
        worst = np.maximum(worst, np.abs(a[sl] - b[sl]).max(axis=0) / max(np.abs(b[sl]).max(), 1e-300))
    return worst


def kept(cast, ref=None, report=None, sbr=False, lib=None, bits=0):
    """The either-way rule: the dead-band, the drop threshold, floor() and the friction sign are discontinuous, so a character
    whose ORACLE answer changes side under a relative 1e-13 change of its initial state decides nothing about a kernel.  The oracle
    runs again with the initial state scaled by 1 + 1e-13 and by 1 - 1e-13.  -> (M,) bool: False where, after any launch, either
    run changes the character's reason or an integer schedule field (THR_LIM, THR_T0, THR_CNT), or the state moves by more than a
    tenth of the GPU bounds in the sense below.

    The state is a smooth function of the initial state away from those edges, with a gain of 10 - 60 in these casts (the feedback
    gains over u_max; measured: every character moves by 0.3 - 6 e-12 of a state group under the scaling, none taking another
    branch), so the plain difference |f(+) - f(0)| exceeds a tenth of the 1e-11 bound for nearly every character, edge or no edge:
    it cannot tell them apart.  What tells them apart is the part of the response that does not change sign with the perturbation,
    f(+) + f(-) - 2 f(0): second order (1e-26 x curvature) for a smooth response, the full jump if either run crossed an edge.  That
    is held to a tenth of the bounds.  The plain difference is reported (``report``: a dict that receives the worst of both, in
    units of the bounds): it is the casts' conditioning - a few bounds at most, that is a gain below 100 on a relative 1e-13, under
    which the kernels' own rounding (1e-16) stays four orders below the bounds.

    tests/_guidance.py adds: ``sbr`` - the att_guidance message's |sigma_BR| (BSK_T_SBR) under the state bound as well; ``lib`` (a
    branch-mask build) and ``bits`` - the three runs go through it (``ref`` carries ``mask``) and a kept character takes the same
    branches among ``bits`` in all of them, launch by launch."""
    n_rw = cast.n_rw
    tail = _lib.NF_BASE + n_rw
    ref = (cast.run_oracle() if lib is None else cast.run_oracle(lib=lib)) if ref is None else ref
    ok = np.ones(cast.M, bool)
    ints = slice(tail + _lib.T_THR_LIM, tail + _lib.T_THR_CNT + 1)
    rem = slice(tail + _lib.T_THR_REM, tail + _lib.T_THR_REM + 8)
    cmds = [slice(tail + f, tail + f + 4) for f in (_lib.T_UCMD, _lib.T_UPEND)]
    if sbr:
        cmds = cmds + [slice(tail + _lib.T_SBR, tail + _lib.T_SBR + 1)]         # (CMD_BOUND is the state bound)
    kw = {} if lib is None else {"lib": lib}
    plus, minus = cast.run_oracle(scale=1.0 + 1e-13, **kw), cast.run_oracle(scale=1.0 - 1e-13, **kw)
    worst = {"plain": 0.0, "symmetric": 0.0}
    for p, m, b in zip(plus, minus, ref):
        for a in (p, m):
            ok &= (a["reason"] == b["reason"]) & (a["state"][ints] == b["state"][ints]).all(axis=0)
            if lib is not None:
                ok &= (a["mask"] & np.uint32(bits)) == (b["mask"] & np.uint32(bits))
        for get, bound in ([lambda x, y: column_errors(x, y, n_rw)], STATE_BOUND), ([lambda x, y: np.abs(x[rem] - y[rem]).max(axis=0)], REM_BOUND), \
                ([lambda x, y, c=c: np.abs(x[c] - y[c]).max(axis=0) for c in cmds], CMD_BOUND):
            for fn in get:
                plain = np.maximum(fn(p["state"], b["state"]), fn(m["state"], b["state"]))
                sym = fn(p["state"] + m["state"] - b["state"], b["state"])
                ok &= sym <= 0.1 * bound
                worst["plain"], worst["symmetric"] = max(worst["plain"], float((plain / bound).max())), max(worst["symmetric"], float((sym / bound).max()))
    if report is not None:
        report.update(worst)
    return ok


def check_cap(cast, ok, exempt=()):
    """At most 2 % left out, every slot keeps 12 of 16 (48 of 64) -> the share left out.  ``exempt``: slots of edge characters by
    construction (tests/_guidance.py: ``tie``), which count in neither."""
    counted = ~np.isin(cast.slot, exempt)
    share = 1.0 - ok[counted].mean()
    assert share <= 0.02, (cast.kind, share)
    for s in cast.slots:
        if s in exempt:
            continue
        w = cast.where(s)
        assert ok[w].sum() >= 0.75 * w.size, (cast.kind, s, int(ok[w].sum()), w.size)
    return share


# ---------------------------------------------------------------------------------------------------------------- proofs
def waves(index):
    """-> list of character arrays, one per wave of 64 envs of a handle (filler left out)"""
    return [index[w:w + WAVE][index[w:w + WAVE] >= 0] for w in range(0, len(index), WAVE)]


def prove(cast, masklib, verbose=True):
    """The presence conditions of tests/test_actuators_host.py from the branch masks alone -> the table that is printed"""
    cfg, kind = cast.cfg, cast.kind
    runs = cast.run_oracle(lib=masklib)
    plain = cast.run_oracle()
    for a, b in zip(runs, plain):                                      # the instrumented build computes the same bits
        for key in b:
            assert np.array_equal(a[key].view(np.uint64) if a[key].dtype == np.float64 else a[key], b[key].view(np.uint64) if b[key].dtype == np.float64 else b[key]), key
    mask = np.array([r["mask"] for r in runs])                          # (launches, M)
    has = {name: (mask & BIT[name]) != 0 for name in BITS}
    ever = {name: has[name].any(axis=0) for name in BITS}
    lines = ["%-16s %s" % ("bit", " ".join("%7s" % s[:7] for s in cast.slots))]
    for name in BITS:
        lines.append("%-16s %s" % (name, " ".join("%7d" % int(ever[name][cast.where(s)].sum()) for s in cast.slots)))
        if name in CARRIED[kind]:
            assert ever[name].sum() >= 8, (kind, name, int(ever[name].sum()))
        else:
            assert not ever[name].any(), (kind, name)
    lay = cast.layouts()
    srt, mixed = waves(lay["sorted"]), waves(lay["mixed"])

    def every_lane(pred, what):                                         # (launches, M) or (M,)
        full = [w for w in srt if w.size == WAVE]
        found = any((pred[..., w].all(axis=-1)).any() for w in full)
        assert found, (kind, what, "in every lane of no wave of sorted")

    every_lane(has["om_zero"], "wheel at rest")
    every_lane(ever["om_cross"], "sign change within the schedule")
    if kind == "desat":
        every_lane(has["thr_stage"], "thruster active in a stage")
        every_lane(has["thr_end"], "burst ending inside a step")
        on = has["thr_stage"]
        assert any(((~on[:, w]).all(axis=1) & np.array([any(on[c, v].any() for v in srt) for c in range(len(KS))])).any() for w in srt), "no wave without a burst beside one with"
        for w in mixed:
            assert (on[:, w].any(axis=1) & (~on[:, w]).any(axis=1)).any(), "a wave of mixed without both"
        # t0 under nav_lag = 1: the request of the t = 0 tick reads empty messages - nothing above hs_min, every pulse empty; and the
        # K = 3 launch holds no FSW tick for a character that started at tick 0: no request at all
        t0 = cast.where("t0")
        assert cfg.nav_lag == 1 and KS[2] == 3
        assert has["req_below"][0, t0].all() and not has["req_above"][0, t0].any() and not (has["thr_stage"][0, t0]).any()
        assert not (mask[0, t0] & (BIT["pulse_drop_owed"] | BIT["pulse_full"] | BIT["pulse_stretch"] | BIT["pulse_partial"])).any()
        assert not (mask[2, t0] & (BIT["req_above"] | BIT["req_below"] | BIT["tick_fire"] | BIT["tick_count"])).any()
        # the masked reset falls inside a running burst
        tail = _lib.NF_BASE + cast.n_rw
        st, tk = runs[RESET_BEFORE - 1]["state"], runs[RESET_BEFORE - 1]["ticks"]
        lim = st[tail + _lib.T_THR_LIM:tail + _lib.T_THR_LIM + 8].max(axis=0)
        inside = (lim > 0) & (2 * (tk - st[tail + _lib.T_THR_T0]) <= lim)
        assert inside[cast.where("reset")].sum() >= 8, int(inside[cast.where("reset")].sum())
        lims = sorted({int(v) for r in runs for v in np.unique(r["state"][tail + _lib.T_THR_LIM:tail + _lib.T_THR_LIM + 8])})
        lines.append("burst limits latched: %s" % lims)
        assert 12 in lims and 20 in lims and 0 in lims
    if verbose:
        print("\n[%s cast, %d wheels, nav_lag %d] characters that take each branch, per slot\n" % (kind, cast.n_rw, cfg.nav_lag) + "\n".join(lines))
    return runs, lines


# ---------------------------------------------------------------------------------------------------------------- the forms
# id -> (gravity, wheels, level, diagonal hub, BSKGPU_PAIR, BSKGPU_TRI, BSKGPU_SH_FORM, nav_lag, how).  ``None`` for a form switch
# leaves the library's own rule: the pair / three-wave form for launches of at least 16 sub-steps.  ``how``: "step", "halves" (the
# halves form forced on: the K = 1 launches run it) or "rollout" (``bsk_step_n`` rows).
def _forms():
    from basilisk_env_amd._lib import GRAV_PM, GRAV_PM_J2, GRAV_SH
    wheel = {}
    for nav in (0, 1):
        for name, row in (("bare-diag", (GRAV_PM_J2, 4, "bare", True, "0", "0", None, nav, "step")),
                          ("bare-full", (GRAV_PM, 3, "bare", False, "0", "0", None, nav, "step")),
                          ("lds-scratch", (GRAV_PM_J2, 4, "ldss", True, "0", "0", None, nav, "step")),
                          ("rollout", (GRAV_PM, 3, "bare", False, "0", "0", None, nav, "rollout")),
                          ("power", (GRAV_PM_J2, 4, "power", True, "0", "0", None, nav, "step")),
                          ("power-pair", (GRAV_PM_J2, 3, "power", True, None, "0", None, nav, "step"))):
            wheel["%s/nav%d" % (name, nav)] = row
    wheel["halves/nav1"] = (GRAV_PM_J2, 4, "bare", True, "0", "0", None, 1, "halves")      # (the form is complete under nav_lag = 1 only)
    desat = {"scenario-diag": (GRAV_PM_J2, 3, "full", True, "0", "0", None, 1, "step"),
             "scenario-full": (GRAV_PM_J2, 3, "full", False, "0", "0", None, 1, "step"),
             "pair": (GRAV_PM_J2, 3, "full", True, None, "0", None, 1, "step"),
             "tri": (GRAV_PM, 4, "full", True, "0", None, None, 1, "step"),
             "generic-facets": (GRAV_PM_J2, 4, "fullg", True, "0", "0", None, 1, "step"),
             "sh-dpp": (GRAV_SH, 3, "full", True, "0", "0", "4", 1, "step"),
             "sh-dpp2": (GRAV_SH, 4, "full", True, "0", "0", "5", 1, "step")}
    return wheel, desat


WHEEL_FORMS, DESAT_FORMS = _forms()
_CASTS = {}


def cast_for(kind, form, forms=None, edit=None, make=None):
    """(cfg, Cast, row) of one entry of WHEEL_FORMS / DESAT_FORMS; built once per session (casts of equal configs are shared).
    tests/_guidance.py passes its own table of ``forms``, config ``edit`` and cast class ``make``."""
    import test_gpu_kernel_info as KI
    from basilisk_env_amd._lib import GRAV_SH
    from helpers import visible_sh_coefficients
    row = (forms if forms is not None else WHEEL_FORMS if kind == "wheel" else DESAT_FORMS)[form]
    edit = (desat_config if kind == "desat" else None) if edit is None else edit
    grav, n_rw, level, diag, _, _, _, nav, _ = row
    key = (kind, grav, n_rw, "bare" if level == "ldss" else level, diag, nav)
    cfg = KI.config(grav, n_rw, level, diag)
    cfg.nav_lag = nav
    if edit is not None:
        edit(cfg)
    if key not in _CASTS:
        ref_cfg = KI.config(grav, n_rw, "bare" if level == "ldss" else level, diag)       # (the LDS-scratch flag changes no arithmetic)
        ref_cfg.nav_lag = nav
        if edit is not None:
            edit(ref_cfg)
        sh = visible_sh_coefficients(ref_cfg.sh_degree, seed=3) if grav == GRAV_SH else (None, None)
        _CASTS[key] = (Cast if make is None else make)(ref_cfg, kind, sh)
    return cfg, _CASTS[key], row


def names_for(cfg, row):
    """{K: the kernel name a launch of K sub-steps must report}"""
    import _config_space as CS
    grav, n_rw, level, diag, pair, tri, sh_form, _, how = row
    hub = "diag" if diag else "full"
    single = CS.kernel_name(cfg, hub, level, "single", sh_form)
    if how == "rollout":
        return {k: CS.kernel_name(cfg, hub, level, rollout="actions") for k in set(KS)}
    out = {k: single for k in set(KS)}
    for k in set(KS):
        if k >= 16 and (pair is None or tri is None):
            out[k] = CS.kernel_name(cfg, hub, level, "pair" if pair is None else "tri", sh_form)
        if k == 1 and how == "halves":
            out[k] = CS.kernel_name(cfg, hub, level, "halves", sh_form)
    return out
